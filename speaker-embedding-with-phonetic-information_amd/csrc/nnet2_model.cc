#include "nnet2_model.h"

#include <ctype.h>

#include <algorithm>

namespace xv {

namespace {

std::string SlurpFile(const std::string& rxfilename) {
  Input in;
  in.Open(rxfilename);
  std::string bytes;
  for (;;) {
    const size_t have = bytes.size(), want = std::max<size_t>(1 << 20, have);
    bytes.resize(have + want);
    const size_t got = in.ReadUpTo(&bytes[have], want);
    bytes.resize(have + got);
    if (got < want) break;
  }
  const int status = in.Close();
  if (bytes.empty())
    throw KioError("no model data read from '" + rxfilename + "'" + (status ? " (input command exited with status " + std::to_string(status) + ")" : ""));
  return bytes;
}

// Kaldi's WriteIntegerVector: binary a size byte 4, a raw int32 count and the values; text "[ a b c ]".
void ReadIntVector(Input& in, bool binary, std::vector<int32_t>* v) {
  v->clear();
  if (binary) {
    if (in.Get() != 4) throw KioError("expected an int32 vector (size byte 4) in " + in.Name());
    int32_t n = 0;
    in.Read(&n, 4);
    if (n < 0 || n > (1 << 24)) throw KioError("implausible integer vector of " + std::to_string(n) + " elements in " + in.Name());
    v->resize((size_t)n);
    if (n) in.Read(v->data(), (size_t)n * 4);
    return;
  }
  int c;
  while ((c = in.Peek()) >= 0 && isspace(c)) in.Get();
  if (in.Get() != '[') throw KioError("expected '[' in front of an integer vector in " + in.Name());
  for (;;) {
    std::string w;
    ReadToken(in, false, &w);
    if (w == "]") return;
    char* end = nullptr;
    const long x = strtol(w.c_str(), &end, 10);
    if (end == w.c_str() || *end) throw KioError("bad integer '" + w + "' in an integer vector in " + in.Name());
    v->push_back((int32_t)x);
  }
}

bool IsAffine(const std::string& t) {
  return t == "AffineComponent" || t == "AffineComponentPreconditioned" || t == "AffineComponentPreconditionedOnline" || t == "FixedAffineComponent";
}
bool IsDimOnly(const std::string& t) { return t == "RectifiedLinearComponent" || t == "NormalizeComponent" || t == "SoftmaxComponent"; }

std::string Where(size_t i, const Nnet2Component& c) { return "component " + std::to_string(i) + " (" + c.type + ")"; }

Nnet2Component ReadComponent(Input& in, bool binary, size_t index) {
  std::string open;
  ReadToken(in, binary, &open);
  if (open.size() < 3 || open.front() != '<' || open.back() != '>' || open[1] == '/') throw KioError("bad component opening tag " + open);
  Nnet2Component c;
  c.type = open.substr(1, open.size() - 2);
  const bool splice = c.type == "SpliceComponent", pnorm = c.type == "PnormComponent", sumgroup = c.type == "SumGroupComponent";
  if (!splice && !pnorm && !sumgroup && !IsAffine(c.type) && !IsDimOnly(c.type))
    throw KioError("component " + std::to_string(index) + " is a " + c.type + ", which nnet-am-compute does not evaluate (built: SpliceComponent, "
                   "FixedAffineComponent, AffineComponent, AffineComponentPreconditioned, AffineComponentPreconditionedOnline, PnormComponent, "
                   "RectifiedLinearComponent, NormalizeComponent, SoftmaxComponent, SumGroupComponent)");
  const std::string close = "</" + c.type + ">";
  int dim = -1, input_dim = -1, output_dim = -1, left = 0, right = 0, const_dim = 0;
  bool have_context = false, have_lr = false, have_linear = false, have_bias = false;
  double p = 2.0;
  std::vector<float> ignored;
  for (;;) {
    std::string tok;
    ReadToken(in, binary, &tok);
    if (tok == close) break;
    if (tok == "<InputDim>") input_dim = ReadInt32(in, binary);
    else if (tok == "<OutputDim>") output_dim = ReadInt32(in, binary);
    else if (tok == "<Dim>") dim = ReadInt32(in, binary);
    else if (tok == "<ConstComponentDim>") const_dim = ReadInt32(in, binary);
    else if (tok == "<LeftContext>") left = ReadInt32(in, binary), have_context = true;
    else if (tok == "<RightContext>") right = ReadInt32(in, binary), have_context = true;
    else if (tok == "<Context>" || tok == "<Sizes>") ReadIntVector(in, binary, &c.ints);
    else if (tok == "<RankIn>" || tok == "<RankOut>" || tok == "<Rank>" || tok == "<UpdatePeriod>") (void)ReadInt32(in, binary);
    else if (tok == "<LearningRate>") (void)ReadFloatOrDouble(in, binary), have_lr = true;
    else if (tok == "<Alpha>" || tok == "<MaxChange>" || tok == "<NumSamplesHistory>" || tok == "<MaxChangePerSample>" || tok == "<Count>")
      (void)ReadFloatOrDouble(in, binary);
    else if (tok == "<P>") p = ReadFloatOrDouble(in, binary);
    else if (tok == "<IsGradient>") (void)ReadBool(in, binary);
    else if (tok == "<LinearParams>") ReadMatrix(in, binary, &c.linear), have_linear = true;
    else if (tok == "<BiasParams>") ReadVector(in, binary, &c.bias), have_bias = true;
    else if (tok == "<ValueSum>" || tok == "<DerivSum>") ReadVector(in, binary, &ignored);
    else throw KioError(Where(index, c) + ": unexpected token " + tok);
  }
  if (splice) {
    if (c.ints.empty() && have_context) {
      if (left < 0 || right < 0) throw KioError(Where(index, c) + ": negative <LeftContext> or <RightContext>");
      for (int t = -left; t <= right; ++t) c.ints.push_back(t);
    }
    if (input_dim < 1 || c.ints.empty()) throw KioError(Where(index, c) + ": <InputDim> and a context are required");
    for (size_t i = 1; i < c.ints.size(); ++i)
      if (c.ints[i] <= c.ints[i - 1]) throw KioError(Where(index, c) + ": the context must increase");
    if (c.ints.front() > 0 || c.ints.back() < 0 || c.ints.front() < -1000 || c.ints.back() > 1000)
      throw KioError(Where(index, c) + ": a context that does not include the present, or is wider than 1000 frames");
    if ((int)c.ints.size() > kNnet2MaxSpliceOffsets)
      throw KioError(Where(index, c) + ": " + std::to_string(c.ints.size()) + " offsets are more than the " + std::to_string(kNnet2MaxSpliceOffsets) +
                     " the affine kernel takes");
    if (const_dim != 0)
      throw KioError(Where(index, c) + ": const-component-dim=" + std::to_string(const_dim) + " is not built (only 0: no i-vector is appended in the recipes' networks)");
    c.in_dim = input_dim;
    c.out_dim = input_dim * (int)c.ints.size();
  } else if (IsAffine(c.type)) {
    if (!have_linear || !have_bias || c.linear.cm || c.linear.rows < 1 || c.linear.cols < 1 || (int)c.bias.size() != c.linear.rows)
      throw KioError(Where(index, c) + ": <LinearParams> and <BiasParams> of matching sizes are required");
    c.updatable = c.type != "FixedAffineComponent";
    if (c.updatable && !have_lr) throw KioError(Where(index, c) + ": <LearningRate> is missing");
    c.in_dim = c.linear.cols;
    c.out_dim = c.linear.rows;
  } else if (pnorm) {
    if (input_dim < 1 || output_dim < 1) throw KioError(Where(index, c) + ": <InputDim> and <OutputDim> are required");
    if (p != 2.0) throw KioError(Where(index, c) + ": P=" + std::to_string(p) + " is not built (only the 2-norm)");
    if (input_dim % output_dim != 0)
      throw KioError(Where(index, c) + ": input-dim=" + std::to_string(input_dim) + " is not a multiple of output-dim=" + std::to_string(output_dim));
    c.in_dim = input_dim;
    c.out_dim = output_dim;
  } else if (sumgroup) {
    int64_t sum = 0;
    for (int32_t s : c.ints) {
      if (s < 1) throw KioError(Where(index, c) + ": a group of size " + std::to_string(s));
      sum += s;
    }
    if (c.ints.empty() || sum > (1 << 24)) throw KioError(Where(index, c) + ": <Sizes> is empty or implausible");
    c.in_dim = (int)sum;
    c.out_dim = (int)c.ints.size();
  } else {
    if (dim < 1) throw KioError(Where(index, c) + ": <Dim> is required");
    c.in_dim = c.out_dim = dim;
  }
  return c;
}

}  // namespace

void Nnet2Model::ReadFrom(const std::string& rxfilename) { Read(SlurpFile(rxfilename), rxfilename); }

void Nnet2Model::Read(const std::string& bytes, const std::string& name) {
  const bool bin = bytes.size() >= 2 && bytes[0] == 0 && bytes[1] == 'B';
  size_t at = bin ? 2 : 0;
  while (!bin && at < bytes.size() && isspace((unsigned char)bytes[at])) ++at;
  static const char kOpen[] = "<TransitionModel>", kClose[] = "</TransitionModel>";
  if (bytes.compare(at, sizeof kOpen - 1, kOpen) != 0) throw KioError("expected <TransitionModel> at the start of the nnet2 acoustic model " + name);
  const size_t close = bytes.find(kClose, at);
  if (close == std::string::npos) throw KioError("no </TransitionModel> in the nnet2 acoustic model " + name);
  size_t rest = close + sizeof kClose - 1;
  if (rest < bytes.size() && bin && bytes[rest] == ' ') ++rest;   // a binary token is followed by one space
  Input in;
  in.OpenMemory(bytes.data() + rest, bytes.size() - rest);
  ExpectToken(in, bin, "<Nnet>");
  ExpectToken(in, bin, "<NumComponents>");
  const int32_t n = ReadInt32(in, bin);
  if (n < 1 || n > 10000) throw KioError("implausible <NumComponents> " + std::to_string(n) + " in " + name);
  ExpectToken(in, bin, "<Components>");
  components.clear();
  for (int32_t i = 0; i < n; ++i) components.push_back(ReadComponent(in, bin, (size_t)i));
  ExpectToken(in, bin, "</Components>");
  ExpectToken(in, bin, "</Nnet>");
  ReadVector(in, bin, &priors);
  Lower();
}

void Nnet2Model::Lower() {
  layers.clear();
  group_sizes.clear();
  num_updatable = 0;
  parameter_dim = 0;
  left_context = right_context = 0;
  for (size_t i = 0; i < components.size(); ++i) {
    const Nnet2Component& c = components[i];
    if (i && components[i - 1].out_dim != c.in_dim)
      throw KioError("the dimensions do not chain: " + Where(i - 1, components[i - 1]) + " gives " + std::to_string(components[i - 1].out_dim) + ", " + Where(i, c) +
                     " takes " + std::to_string(c.in_dim));
    if (c.updatable) {
      ++num_updatable;
      parameter_dim += (int64_t)c.linear.data.size() + (int64_t)c.bias.size();
    }
  }
  input_dim = components.front().in_dim;
  size_t end = components.size();
  if (components[end - 1].type == "SumGroupComponent") {
    group_sizes = components[end - 1].ints;
    --end;
  }
  if (end < 2 || components[end - 1].type != "SoftmaxComponent")
    throw KioError("the network does not end in SoftmaxComponent [SumGroupComponent] (its last component is " + components.back().type +
                   "): nnet-am-compute gives posteriors only");
  softmax_dim = components[end - 1].out_dim;
  output_dim = components.back().out_dim;
  --end;   // components [0, end) make the layers
  size_t i = 0;
  while (i < end) {
    Nnet2Layer l;
    const Nnet2Component* c = &components[i];
    if (c->type == "SpliceComponent") {
      l.context = c->ints;
      l.in_dim = c->in_dim;
      left_context += -c->ints.front();
      right_context += c->ints.back();
      if (++i == end || !IsAffine(components[i].type))
        throw KioError(Where(i - 1, *c) + " is not followed by an affine component: that order is not built");
      c = &components[i];
    } else {
      l.context.assign(1, 0);
      l.in_dim = c->in_dim;
    }
    if (!IsAffine(c->type)) throw KioError(Where(i, *c) + " does not follow an affine component: that order is not built");
    l.linear = &c->linear;
    l.bias = &c->bias;
    l.affine_dim = l.out_dim = c->out_dim;
    ++i;
    if (i < end && (components[i].type == "PnormComponent" || components[i].type == "RectifiedLinearComponent")) {
      l.nonlin = components[i].type == "PnormComponent" ? kNnet2Pnorm : kNnet2Relu;
      l.out_dim = components[i].out_dim;
      ++i;
    }
    if (i < end && components[i].type == "NormalizeComponent") {
      l.normalize = true;
      ++i;
    }
    layers.push_back(l);
  }
  if (layers.empty() || layers.back().nonlin != kNnet2None || layers.back().normalize)
    throw KioError("the network does not end in an affine component, SoftmaxComponent [SumGroupComponent]: nnet-am-compute gives posteriors only");
  if (softmax_dim > 16384)
    throw KioError("a softmax of " + std::to_string(softmax_dim) + " outputs: more than the 16384 the head kernel holds");
}

std::string Nnet2Model::Info() const {
  std::string s;
  s += "num-components " + std::to_string(components.size()) + "\n";
  s += "num-updatable-components " + std::to_string(num_updatable) + "\n";
  s += "left-context " + std::to_string(left_context) + "\n";
  s += "right-context " + std::to_string(right_context) + "\n";
  s += "input-dim " + std::to_string(input_dim) + "\n";
  s += "output-dim " + std::to_string(output_dim) + "\n";
  s += "parameter-dim " + std::to_string(parameter_dim) + "\n";
  for (size_t i = 0; i < components.size(); ++i) {
    const Nnet2Component& c = components[i];
    s += "component " + std::to_string(i) + " : " + c.type + ", input-dim=" + std::to_string(c.in_dim) + ", output-dim=" + std::to_string(c.out_dim);
    if (c.type == "SpliceComponent") {
      s += ", context=";
      for (size_t k = 0; k < c.ints.size(); ++k) s += (k ? ":" : "") + std::to_string(c.ints[k]);
    }
    s += "\n";
  }
  s += "prior dimension: " + std::to_string(priors.size()) + "\n";
  return s;
}

}  // namespace xv
