// The nnet2 acoustic model (Kaldi's nnet2 `final.mdl`) as nnet-am-compute and nnet-am-info need it: the reader of the file and
// the lowering of its component list to a short program of layers.  Host only: kio.h and the standard library, no device.
//
// The file (binary after "\0B", or text), DESIGN.md section 3.13.1:
//   <TransitionModel> ... </TransitionModel>                      skipped, as nnet3_raw.cc skips it
//   <Nnet> <NumComponents> i32 <Components> component... </Components> </Nnet>
//   priors                                                        a float vector, no token in front of it, possibly empty
// A component is <Type> fields... </Type>.  The types read (everything steps/nnet2/make_multisplice_configs.py and
// train_multisplice_accel2.sh can produce) and their fields:
//   SpliceComponent                       <InputDim> i <Context> int-vector <ConstComponentDim> i
//                                         (older files: <LeftContext> i <RightContext> i in place of <Context>)
//   FixedAffineComponent                  <LinearParams> M <BiasParams> V
//   AffineComponent                       <LearningRate> f <LinearParams> M <BiasParams> V <IsGradient> b
//   AffineComponentPreconditioned         <LearningRate> <LinearParams> <BiasParams> <Alpha> f <MaxChange> f
//   AffineComponentPreconditionedOnline   <LearningRate> <LinearParams> <BiasParams> <RankIn> i <RankOut> i (or one <Rank> i)
//                                         <UpdatePeriod> i <NumSamplesHistory> f <Alpha> f <MaxChangePerSample> f
//   PnormComponent                        <InputDim> i <OutputDim> i <P> f
//   RectifiedLinearComponent, NormalizeComponent, SoftmaxComponent
//                                         <Dim> i <ValueSum> V <DerivSum> V <Count> f     (V float or double, possibly empty)
//   SumGroupComponent                     <Sizes> int-vector
// Refused by name (KioError that names the component): any other type; <ConstComponentDim> other than 0; <P> other than 2; a
// p-norm whose input dimension is no multiple of its output dimension; a network that does not end in SoftmaxComponent
// [SumGroupComponent]; dimensions that do not chain; a splice of more than 32 offsets; a softmax wider than 16384.  Parity with files written by Kaldi itself is unpinned: the grammar is
// restated from nnet2/nnet-component.cc of early 2018, and no such file was at hand.
//
// The program: layers {optional splice (time offsets of the layer's input), affine, one of none / p-norm / ReLU, optional
// normalize}, then the head {softmax, optional group sums, optional priors, optional log}.  Left context = the sum of
// -context.front() over the splices, right context = the sum of context.back().
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "kio.h"

namespace xv {

struct Nnet2Component {
  std::string type;
  int in_dim = 0, out_dim = 0;
  std::vector<int32_t> ints;   // Splice: the context; SumGroup: the sizes
  Matrix linear;               // the affine flavours: [out][in]
  std::vector<float> bias;
  bool updatable = false;
};

constexpr int kNnet2MaxSpliceOffsets = 32;   // what the affine kernel takes (nnet2_kernels.h kNnet2MaxContext)

enum Nnet2Nonlin { kNnet2None = 0, kNnet2Pnorm = 1, kNnet2Relu = 2 };

struct Nnet2Layer {
  std::vector<int32_t> context;   // {0}: no splice
  int in_dim = 0;                 // per time offset: the affine takes context.size() * in_dim
  int affine_dim = 0;             // rows of the affine
  const Matrix* linear = nullptr; // points into Nnet2Model::components
  const std::vector<float>* bias = nullptr;
  int nonlin = kNnet2None;
  int out_dim = 0;                // after the nonlinearity
  bool normalize = false;
};

struct Nnet2Model {
  std::vector<Nnet2Component> components;
  std::vector<float> priors;
  // the lowering
  std::vector<Nnet2Layer> layers;
  std::vector<int32_t> group_sizes;   // empty: no SumGroupComponent
  int input_dim = 0, output_dim = 0, softmax_dim = 0;
  int left_context = 0, right_context = 0;
  int num_updatable = 0;
  int64_t parameter_dim = 0;

  // Reads and lowers; KioError on anything the grammar above does not hold, on a refusal and on a truncated file.
  void ReadFrom(const std::string& rxfilename);
  void Read(const std::string& bytes, const std::string& name);
  // The text nnet-am-info prints.
  std::string Info() const;

 private:
  void Lower();
};

}  // namespace xv
