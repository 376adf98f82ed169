#include "nnet2.h"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "device.h"
#include "nnet2_kernels.h"

namespace xv {

namespace {

static_assert(kNnet2MaxSpliceOffsets == kNnet2MaxContext, "the reader refuses what the affine kernel cannot take");

int RoundUp(int v, int to) { return (v + to - 1) / to * to; }

uint16_t HalfBits(float x) {
  const _Float16 h = (_Float16)x;
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}
float HalfValue(float x) { return (float)(_Float16)x; }

// One affine's weights as the kernel reads them: [n_pad][n_ctx * k_pad] (hi, lo), scaled by a power of two.
struct PackedAffine {
  std::vector<uint16_t> hi, lo;
  int n = 0, n_pad = 0, k = 0, k_pad = 0, n_ctx = 0;
  float unscale = 1.f;
};

PackedAffine PackAffine(const float* w, int n, int k, int n_ctx) {
  PackedAffine p;
  p.n = n;
  p.k = k;
  p.n_ctx = n_ctx;
  p.n_pad = RoundUp(n, kNnet2TileN);
  p.k_pad = RoundUp(k, kNnet2TileK);
  float mx = 0.f;
  const size_t total = (size_t)n * n_ctx * k;
  for (size_t i = 0; i < total; ++i)
    if (fabsf(w[i]) > mx && isfinite(w[i])) mx = fabsf(w[i]);
  int e = 14;
  if (mx > 0.f) (void)frexpf(mx, &e);   // mx in [2^(e-1), 2^e)
  const float scale = ldexpf(1.f, 14 - e);
  p.unscale = ldexpf(1.f, e - 14);
  const size_t ldw = (size_t)n_ctx * p.k_pad;
  p.hi.assign((size_t)p.n_pad * ldw, 0);
  p.lo.assign((size_t)p.n_pad * ldw, 0);
  for (int j = 0; j < n; ++j)
    for (int c = 0; c < n_ctx; ++c)
      for (int i = 0; i < k; ++i) {
        const float v = w[((size_t)j * n_ctx + c) * k + i] * scale;
        const float h = HalfValue(v);
        const size_t at = (size_t)j * ldw + (size_t)c * p.k_pad + i;
        p.hi[at] = HalfBits(v);
        p.lo[at] = HalfBits((v - h) * kNnet2LoScale);
      }
  return p;
}

struct DeviceAffine {
  DevBuf hi, lo, bias;
  int n = 0, n_pad = 0, k_pad = 0, n_ctx = 0;
  float unscale = 1.f;
  int ctx[kNnet2MaxContext] = {0};
  void Upload(const PackedAffine& p, const float* b, const int32_t* context) {
    hi.Upload(p.hi, "copy the weights");
    lo.Upload(p.lo, "copy the weights");
    bias.Upload(b, (size_t)p.n * 4, "copy the bias");
    n = p.n;
    n_pad = p.n_pad;
    k_pad = p.k_pad;
    n_ctx = p.n_ctx;
    unscale = p.unscale;
    for (int c = 0; c < n_ctx; ++c) ctx[c] = context[c];
  }
  Nnet2AffineArgs Args(const uint16_t* x_hi, const uint16_t* x_lo, int rows, int row_lo, int row_hi, float* out, int ldo) const {
    Nnet2AffineArgs a{};
    a.x_hi = x_hi;
    a.x_lo = x_lo;
    a.ldx = k_pad;
    a.rows = rows;
    a.row_lo = row_lo;
    a.row_hi = row_hi;
    a.n_ctx = n_ctx;
    for (int c = 0; c < n_ctx; ++c) a.ctx[c] = ctx[c];
    a.k_pad = k_pad;
    a.w_hi = hi.as<uint16_t>();
    a.w_lo = lo.as<uint16_t>();
    a.n_pad = n_pad;
    a.n = n;
    a.bias = bias.as<float>();
    a.w_unscale = unscale;
    a.out = out;
    a.ldo = ldo;
    return a;
  }
};

std::vector<int32_t> GroupStarts(const int32_t* sizes, int n_groups) {
  std::vector<int32_t> start((size_t)n_groups + 1, 0);
  for (int g = 0; g < n_groups; ++g) start[(size_t)g + 1] = start[(size_t)g] + sizes[g];
  return start;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ the plan
Nnet2Dims DimsOf(const Nnet2Model& m) {
  Nnet2Dims d;
  d.input_dim = m.input_dim;
  d.output_dim = m.output_dim;
  d.softmax_dim = m.softmax_dim;
  d.left_context = m.left_context;
  d.right_context = m.right_context;
  for (const Nnet2Layer& l : m.layers) {
    d.max_plane_cols = std::max(d.max_plane_cols, RoundUp(l.in_dim, kNnet2TileK));
    d.max_pre_cols = std::max(d.max_pre_cols, l.affine_dim);
    d.halo = std::max(d.halo, std::max(-l.context.front(), l.context.back()));
  }
  return d;
}

int64_t Nnet2BlockBytes(const Nnet2Dims& d, int64_t block_rows) {
  const int64_t n = block_rows + d.left_context + d.right_context;
  return 2 * (n + 2 * d.halo) * d.max_plane_cols * 2 + n * (int64_t)d.max_pre_cols * 4 + n * (int64_t)d.input_dim * 4 + block_rows * ((int64_t)d.output_dim * 4 + 4);
}

bool Nnet2Plan(const Nnet2Dims& d, int64_t rows, int64_t block_rows, int64_t workspace_bytes, Nnet2BlockPlan* plan, std::string* why) {
  *plan = Nnet2BlockPlan();
  if (rows < 0 || d.input_dim < 1 || d.output_dim < 1 || d.max_plane_cols < 1 || d.max_pre_cols < 1 || d.left_context < 0 || d.right_context < 0 || d.halo < 0) {
    *why = "bad argument";
    return false;
  }
  if (block_rows > kNnet2MaxBlockRows) {
    *why = "a block of " + std::to_string(block_rows) + " rows is more than the " + std::to_string(kNnet2MaxBlockRows) + " of one launch";
    return false;
  }
  const int64_t cap = workspace_bytes > 0 ? workspace_bytes : kNnet2DefaultWorkspace;
  // bytes(B) = fixed + per_row B
  const int64_t fixed = Nnet2BlockBytes(d, 0), per_row = Nnet2BlockBytes(d, 1) - fixed;
  int64_t b = block_rows;
  if (b <= 0) {
    b = std::min<int64_t>((cap - fixed) / per_row, kNnet2MaxBlockRows);
    if (rows > 0) b = std::min(b, rows);   // no more than the sequence has
    else b = std::min<int64_t>(b, 1);
  }
  if (b < 1 || Nnet2BlockBytes(d, b) > cap) {
    *why = "a workspace of " + std::to_string(cap) + " bytes does not hold " + (block_rows > 0 ? "a block of " + std::to_string(block_rows) + " rows" : std::string("one row")) +
           " with its " + std::to_string(d.left_context + d.right_context) + " rows of context (" + std::to_string(Nnet2BlockBytes(d, std::max<int64_t>(b, 1))) + " bytes)";
    return false;
  }
  plan->rows_per_block = b;
  plan->n_blocks = CeilDiv(rows, b);
  plan->bytes = rows > 0 ? Nnet2BlockBytes(d, b) : 0;
  return true;
}

// ----------------------------------------------------------------------------------------------------------------------- the model
struct Nnet2::Device {
  int device = -1;
  std::vector<std::unique_ptr<DeviceAffine>> affine;
  DevBuf start, inv_prior;
  DevBuf planes, pre, in, out, map;
  int64_t planes_bytes = 0;
};

Nnet2::Nnet2(const std::string& rxfilename) {
  model_.ReadFrom(rxfilename);
  dims_ = DimsOf(model_);
}

Nnet2::~Nnet2() {}

int64_t Nnet2::OutRows(int64_t t, int flags) const {
  if (t <= 0) return 0;
  if (flags & kNnet2PadInput) return t;
  return std::max<int64_t>(0, t - dims_.left_context - dims_.right_context);
}

void Nnet2::CheckFlags(int flags) const {
  if (flags & ~(kNnet2ApplyLog | kNnet2DivideByPriors | kNnet2PadInput)) throw Nnet2ArgError("nnet-am-compute: unknown flags");
  if ((flags & kNnet2DivideByPriors) && (int)model_.priors.size() != model_.output_dim)
    throw Nnet2ArgError(model_.priors.empty() ? std::string("--divide-by-priors=true, but the model has no priors")
                                              : "--divide-by-priors=true, but the model has " + std::to_string(model_.priors.size()) + " priors for " +
                                                    std::to_string(model_.output_dim) + " outputs");
}

void Nnet2::Upload(int device) {
  UseDevice(device, "nnet-am-compute needs");
  if (dev_ && dev_->device == device) return;
  std::unique_ptr<Device> d(new Device);
  d->device = device;
  d->affine.resize(model_.layers.size());
  for (size_t i = 0; i < model_.layers.size(); ++i) {
    const Nnet2Layer& l = model_.layers[i];
    const PackedAffine p = PackAffine(l.linear->Data(), l.affine_dim, l.in_dim, (int)l.context.size());
    d->affine[i].reset(new DeviceAffine);
    d->affine[i]->Upload(p, l.bias->data(), l.context.data());
  }
  if (!model_.group_sizes.empty()) d->start.Upload(GroupStarts(model_.group_sizes.data(), (int)model_.group_sizes.size()), "copy the group starts");
  if ((int)model_.priors.size() == model_.output_dim) {
    std::vector<float> inv(model_.priors.size());
    for (size_t j = 0; j < inv.size(); ++j) inv[j] = 1.f / model_.priors[j];
    d->inv_prior.Upload(inv, "copy the priors");
  }
  dev_ = std::move(d);
}

void Nnet2::Compute(int device, const float* feats, const int32_t* row_off, int n_utts, int flags, int64_t block_rows, float* out, float* device_ms,
                    float* layer_ms) {
  const int L = dims_.left_context, R = dims_.right_context, H = dims_.halo, D = dims_.input_dim;
  if (!row_off || n_utts < 0) throw Nnet2ArgError("nnet-am-compute: bad argument");
  if (row_off[0] != 0) throw Nnet2ArgError("nnet-am-compute: row offsets must start at 0");
  for (int u = 0; u < n_utts; ++u)
    if (row_off[u + 1] < row_off[u]) throw Nnet2ArgError("nnet-am-compute: row offsets must not decrease");
  if (row_off[n_utts] > 0 && (!feats || !out)) throw Nnet2ArgError("nnet-am-compute: bad argument");
  CheckFlags(flags);
  const bool pad = (flags & kNnet2PadInput) != 0;
  // the packed sequence of extended utterances
  std::vector<int64_t> eoff((size_t)n_utts + 1, 0);
  for (int u = 0; u < n_utts; ++u) {
    const int64_t t = row_off[u + 1] - row_off[u];
    eoff[(size_t)u + 1] = eoff[(size_t)u] + (OutRows(t, flags) > 0 ? (pad ? t + L + R : t) : 0);
  }
  const int64_t S = eoff.back();
  const size_t n_layers = model_.layers.size();
  if (device_ms) *device_ms = 0.f;
  if (layer_ms) std::fill(layer_ms, layer_ms + n_layers + 1, 0.f);
  Nnet2BlockPlan plan;
  std::string why;
  if (!Nnet2Plan(dims_, S, block_rows, 0, &plan, &why)) throw Nnet2ArgError("nnet-am-compute: " + why);
  Upload(device);   // also with nothing to do: a call without a device fails the same way whatever it is given
  if (S == 0) return;
  Device& dv = *dev_;
  const int64_t B = plan.rows_per_block, n_max = B + L + R;
  const size_t plane_bytes = (size_t)(n_max + 2 * H) * dims_.max_plane_cols * 2;
  if ((int64_t)(2 * plane_bytes) > dv.planes_bytes) {
    dv.planes.Alloc(2 * plane_bytes);
    Check(hipMemset(dv.planes.p, 0, 2 * plane_bytes), "hipMemset");
    dv.planes_bytes = (int64_t)(2 * plane_bytes);
  }
  // hi at the start, lo half way: of the CURRENT allocation, which may be larger than this call needs
  uint16_t* const hi0 = dv.planes.as<uint16_t>();
  uint16_t* const lo0 = hi0 + (size_t)dv.planes_bytes / 4;
  dv.pre.Reserve((size_t)n_max * dims_.max_pre_cols * 4);
  dv.in.Reserve((size_t)n_max * D * 4);
  dv.out.Reserve((size_t)B * dims_.output_dim * 4);
  dv.map.Reserve((size_t)B * 4);
  const bool timed = device_ms || layer_ms;
  std::vector<float> stage((size_t)n_max * D);
  std::vector<int32_t> src_row;
  int u = 0;   // the utterance that holds the row we are at
  int64_t out_done = 0;
  for (int64_t blk = 0; blk < plan.n_blocks; ++blk) {
    const int64_t b0 = blk * B, b1 = std::min(S, b0 + B);
    const int64_t i0 = std::max<int64_t>(0, b0 - L), i1 = std::min(S, b1 + R);
    const int n = (int)(i1 - i0);
    // the input rows [i0, i1) and the rows of [b0, b1) that are outputs
    while (eoff[(size_t)u + 1] <= i0) ++u;
    src_row.clear();
    int v = u;
    for (int64_t p = i0; p < i1; ++p) {
      while (eoff[(size_t)v + 1] <= p) ++v;
      const int64_t e = p - eoff[(size_t)v], t = row_off[v + 1] - row_off[v], ext = eoff[(size_t)v + 1] - eoff[(size_t)v];
      const int64_t s = pad ? std::min(std::max<int64_t>(e - L, 0), t - 1) : e;
      memcpy(&stage[(size_t)(p - i0) * D], feats + (size_t)(row_off[v] + s) * D, (size_t)D * 4);
      if (p >= b0 && p < b1 && e >= L && e < ext - R) src_row.push_back((int32_t)(p - i0));
    }
    const int n_out_rows = (int)src_row.size();
    Check(hipMemcpy(dv.in.p, stage.data(), (size_t)n * D * 4, hipMemcpyHostToDevice), "copy the features");
    if (n_out_rows) Check(hipMemcpy(dv.map.p, src_row.data(), (size_t)n_out_rows * 4, hipMemcpyHostToDevice), "copy the row map");
    EventTimer timer(timed, (int)n_layers + 2);
    timer.Mark();
    for (size_t i = 0; i < n_layers; ++i) {
      const Nnet2Layer& l = model_.layers[i];
      const DeviceAffine& a = *dv.affine[i];
      uint16_t* hi = hi0 + (size_t)H * a.k_pad;
      uint16_t* lo = lo0 + (size_t)H * a.k_pad;
      if (i == 0) {
        Nnet2PrepArgs pa{dv.in.as<float>(), n, D, hi, lo, a.k_pad};
        Check(launch_nnet2_prep(pa, nullptr), "nnet2_prep");
      } else {
        const Nnet2Layer& prev = model_.layers[i - 1];
        Nnet2RowArgs ra{};
        ra.pre = dv.pre.as<float>();
        ra.rows = n;
        ra.ldp = prev.affine_dim;
        ra.in_dim = prev.affine_dim;
        ra.out_dim = prev.out_dim;
        ra.nonlin = prev.nonlin;
        ra.normalize = prev.normalize ? 1 : 0;
        ra.hi = hi;
        ra.lo = lo;
        ra.ld = a.k_pad;
        Check(launch_nnet2_row(ra, nullptr), "nnet2_row");
      }
      Check(launch_nnet2_affine(a.Args(hi, lo, n, -H, n + H, dv.pre.as<float>(), l.affine_dim), nullptr), "nnet2_affine");
      timer.Mark();
    }
    Nnet2HeadArgs ha{};
    ha.logits = dv.pre.as<float>();
    ha.ldl = ha.n = dims_.softmax_dim;
    ha.src_row = dv.map.as<int32_t>();
    ha.rows = n_out_rows;
    ha.start = model_.group_sizes.empty() ? nullptr : dv.start.as<int32_t>();
    ha.n_out = dims_.output_dim;
    ha.inv_prior = (flags & kNnet2DivideByPriors) ? dv.inv_prior.as<float>() : nullptr;
    ha.apply_log = (flags & kNnet2ApplyLog) ? 1 : 0;
    ha.out = dv.out.as<float>();
    Check(launch_nnet2_head(ha, nullptr), "nnet2_head");
    timer.Mark();
    dv.out.Download(out + (size_t)out_done * dims_.output_dim, (size_t)n_out_rows * dims_.output_dim * 4, "copy the posteriors");
    out_done += n_out_rows;
    if (timed)
      for (size_t i = 0; i <= n_layers; ++i) {
        const float ms = timer.Span(i);
        if (layer_ms) layer_ms[i] += ms;
        if (device_ms) *device_ms += ms;
      }
  }
  Check(hipDeviceSynchronize(), "nnet-am-compute");
}

// ------------------------------------------------------------------------------------------------- one launch each, for the tests
void Nnet2KernelAffine(int device, const float* x, int rows, int k, const int32_t* context, int n_ctx, const float* w, const float* bias, int n, float* out) {
  if (rows < 1 || k < 1 || n < 1 || n_ctx < 1 || n_ctx > kNnet2MaxContext || !x || !context || !w || !bias || !out)
    throw Nnet2ArgError("xv_nnet2_kernel_affine: bad argument");
  int halo = 0;
  for (int c = 0; c < n_ctx; ++c) {
    if (c && context[c] <= context[c - 1]) throw Nnet2ArgError("xv_nnet2_kernel_affine: the context must increase");
    halo = std::max(halo, std::abs(context[c]));
  }
  if (halo > 1000) throw Nnet2ArgError("xv_nnet2_kernel_affine: a context wider than 1000 frames");
  UseDevice(device, "nnet-am-compute needs");
  const PackedAffine p = PackAffine(w, n, k, n_ctx);
  DeviceAffine a;
  a.Upload(p, bias, context);
  const size_t plane = (size_t)(rows + 2 * halo) * p.k_pad * 2;
  DevBuf hi(plane), lo(plane), dx((size_t)rows * k * 4), dout((size_t)rows * n * 4);
  Check(hipMemset(hi.p, 0, plane), "hipMemset");
  Check(hipMemset(lo.p, 0, plane), "hipMemset");
  dx.Upload(x, (size_t)rows * k * 4, "copy the input");
  uint16_t* h = hi.as<uint16_t>() + (size_t)halo * p.k_pad;
  uint16_t* l = lo.as<uint16_t>() + (size_t)halo * p.k_pad;
  Nnet2PrepArgs pa{dx.as<float>(), rows, k, h, l, p.k_pad};
  Check(launch_nnet2_prep(pa, nullptr), "nnet2_prep");
  Check(launch_nnet2_affine(a.Args(h, l, rows, -halo, rows + halo, dout.as<float>(), n), nullptr), "nnet2_affine");
  Check(hipDeviceSynchronize(), "nnet2_affine");
  dout.Download(out, (size_t)rows * n * 4, "copy the output");
}

void Nnet2KernelRow(int device, const float* pre, int rows, int in_dim, int out_dim, int nonlin, bool normalize, uint16_t* hi, uint16_t* lo) {
  if (rows < 1 || in_dim < 1 || out_dim < 1 || nonlin < 0 || nonlin > 2 || !pre || !hi || !lo || (nonlin == kNnet2Pnorm ? in_dim % out_dim != 0 : in_dim != out_dim))
    throw Nnet2ArgError("xv_nnet2_kernel_row: bad argument");
  UseDevice(device, "nnet-am-compute needs");
  const int ld = RoundUp(out_dim, kNnet2TileK);
  DevBuf dp((size_t)rows * in_dim * 4), dh((size_t)rows * ld * 2), dl((size_t)rows * ld * 2);
  dp.Upload(pre, (size_t)rows * in_dim * 4, "copy the input");
  Nnet2RowArgs ra{};
  ra.pre = dp.as<float>();
  ra.rows = rows;
  ra.ldp = in_dim;
  ra.in_dim = in_dim;
  ra.out_dim = out_dim;
  ra.nonlin = nonlin;
  ra.normalize = normalize ? 1 : 0;
  ra.hi = dh.as<uint16_t>();
  ra.lo = dl.as<uint16_t>();
  ra.ld = ld;
  Check(launch_nnet2_row(ra, nullptr), "nnet2_row");
  Check(hipDeviceSynchronize(), "nnet2_row");
  dh.Download(hi, (size_t)rows * ld * 2, "copy the output");
  dl.Download(lo, (size_t)rows * ld * 2, "copy the output");
}

void Nnet2KernelHead(int device, const float* logits, int rows, int n, const int32_t* sizes, int n_groups, const float* priors, bool apply_log, float* out) {
  if (rows < 1 || n < 1 || n > kNnet2HeadMaxCols || !logits || !out || (sizes && n_groups < 1)) throw Nnet2ArgError("xv_nnet2_kernel_head: bad argument");
  const int n_out = sizes ? n_groups : n;
  std::vector<int32_t> start;
  if (sizes) {
    for (int g = 0; g < n_groups; ++g)
      if (sizes[g] < 1) throw Nnet2ArgError("xv_nnet2_kernel_head: a group of size " + std::to_string(sizes[g]));
    start = GroupStarts(sizes, n_groups);
    if (start.back() != n) throw Nnet2ArgError("xv_nnet2_kernel_head: the group sizes do not sum to the width");
  }
  UseDevice(device, "nnet-am-compute needs");
  DevBuf dx((size_t)rows * n * 4), dout((size_t)rows * n_out * 4), dstart, dprior;
  dx.Upload(logits, (size_t)rows * n * 4, "copy the input");
  if (sizes) dstart.Upload(start, "copy the group starts");
  if (priors) {
    std::vector<float> inv((size_t)n_out);
    for (int j = 0; j < n_out; ++j) inv[(size_t)j] = 1.f / priors[j];
    dprior.Upload(inv, "copy the priors");
  }
  Nnet2HeadArgs ha{};
  ha.logits = dx.as<float>();
  ha.ldl = ha.n = n;
  ha.rows = rows;
  ha.start = sizes ? dstart.as<int32_t>() : nullptr;
  ha.n_out = n_out;
  ha.inv_prior = priors ? dprior.as<float>() : nullptr;
  ha.apply_log = apply_log ? 1 : 0;
  ha.out = dout.as<float>();
  Check(launch_nnet2_head(ha, nullptr), "nnet2_head");
  Check(hipDeviceSynchronize(), "nnet2_head");
  dout.Download(out, (size_t)rows * n_out * 4, "copy the output");
}

}  // namespace xv
