// extern "C" boundary of libxvec_hip.so - see include/xvec_hip.h and include/xvec_hip_asnorm.h.
#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/xvec_hip.h"
#include "../../include/xvec_hip_asnorm.h"
#include "../../include/xvec_hip_nnet2.h"
#include "backend.h"
#include "cmvn.h"
#include "compress.h"
#include "device.h"
#include "engine.h"
#include "extractor.h"
#include "feat.h"
#include "reverb.h"
#include "wave.h"
#include "kernels.h"
#include "gemm_plan.h"
#include "calib_file.h"
#include "fuse_pipe.h"
#include "fuse_wav.h"
#include "multi_gpu.h"
#include "nnet2.h"
#include "nnet2_kernels.h"
#include "nnet3_raw.h"
#include "plda.h"
#include "plda_kernels.h"
#include "plda_dense_kernels.h"
#include "post.h"
#include "program.h"
#include "table_extract.h"
#include "ivex.h"
#include "ivex_train.h"
#include "ubm.h"
#include "gmm_classify.h"
#include "dubm_train.h"
#include "ubm_train.h"
#include "ubm_train_kernels.h"

struct xv_model {
  xv::TdnnProgram prog;
};

struct xv_ctx {
  std::unique_ptr<xv::Engine> eng;
  bool calibrate = false;       // xv_ctx_set_calibration: table jobs calibrate on the head of their table first
  float calibrate_tol = 7.5e-5f;   // three quarters of the 1e-4 bar, on the WORST calibration chunk
  std::string calibration_file;    // xv_ctx_set_calibration_file: the shared choice of the recipe (calib_file.h)
};

namespace {

thread_local std::string g_err;

xv_status Fail(xv_status s, const std::string& m) {
  g_err = m;
  return s;
}

template <class F>
xv_status Guard(F&& f) {
  try {
    g_err.clear();
    return f();
  } catch (const xv::KioError& e) {
    return Fail(XV_ERR_IO, e.what());
  } catch (const xv::EngineError& e) {
    return Fail(XV_ERR_DEVICE, e.what());
  } catch (const std::bad_alloc&) {
    return Fail(XV_ERR_INTERNAL, "out of host memory");
  } catch (const std::exception& e) {
    return Fail(XV_ERR_INTERNAL, e.what());
  } catch (...) {
    return Fail(XV_ERR_INTERNAL, "unknown exception");
  }
}

void FillInfo(const xv::BlobInfo& b, xv_model_info_t* info) {
  memset(info, 0, sizeof *info);
  info->input_dim = b.input_dim;
  info->output_dim = b.output_dim;
  info->left_context = b.left_context;
  info->right_context = b.right_context;
  info->min_frames = b.min_frames;
  info->num_layers = (int32_t)b.layers.size();
  info->output_is_segment = b.output_is_segment;
}

xv_status LoadCommon(xv::RawNnet& net, const char* nnet_config, const char* output_node, xv_model** out) {
  if (nnet_config && *nnet_config) net.ApplyNnetConfig(nnet_config);
  std::unique_ptr<xv_model> m(new xv_model);
  try {
    m->prog = xv::LowerToProgram(net, output_node && *output_node ? output_node : "output");
  } catch (const xv::KioError& e) {
    return Fail(XV_ERR_MODEL, e.what());
  }
  *out = m.release();
  return XV_OK;
}

}  // namespace

extern "C" {

const char* xv_last_error(void) { return g_err.c_str(); }
// XVEC_KERNELS_SHA: first 16 hex digits of the SHA-1 of kernels.hip + kernels.h this library was built from (Makefile; the stamp
// tools/parse_rocprof.py puts on profiles/pmc_traffic.json): tells a stale or a differently configured build of the library from
// the tree's (tests/test_gpu_fuzz.py compares the product and the schedule-fuzzing build with it).
#ifndef XVEC_KERNELS_SHA
#define XVEC_KERNELS_SHA "unknown"
#endif
#ifdef XVEC_SCHED_FUZZ
#define XVEC_BUILD_KIND "; schedule-fuzzing build"
#else
#define XVEC_BUILD_KIND ""
#endif
const char* xv_version(void) { return "xvec_hip 0.4 (gfx950; kernels " XVEC_KERNELS_SHA XVEC_BUILD_KIND ")"; }

xv_status xv_model_load(const void* raw, size_t n, const char* nnet_config, const char* output_node, xv_model** out) {
  if (!raw || !out) return Fail(XV_ERR_ARG, "xv_model_load: null argument");
  return Guard([&] {
    xv::RawNnet net;
    net.Read(std::string((const char*)raw, n));
    return LoadCommon(net, nnet_config, output_node, out);
  });
}

xv_status xv_model_load_rxfilename(const char* rxfilename, const char* nnet_config, const char* output_node,
                                   xv_model** out) {
  if (!rxfilename || !out) return Fail(XV_ERR_ARG, "xv_model_load_rxfilename: null argument");
  return Guard([&] {
    xv::RawNnet net;
    net.ReadFrom(rxfilename);
    return LoadCommon(net, nnet_config, output_node, out);
  });
}

void xv_model_free(xv_model* m) { delete m; }

xv_status xv_model_info(const xv_model* m, xv_model_info_t* info) {
  if (!m || !info) return Fail(XV_ERR_ARG, "xv_model_info: null argument");
  memset(info, 0, sizeof *info);
  info->input_dim = m->prog.input_dim;
  info->output_dim = m->prog.output_dim;
  info->left_context = m->prog.left_context;
  info->right_context = m->prog.right_context;
  info->min_frames = m->prog.min_frames;
  info->num_layers = (int32_t)m->prog.layers.size();
  info->output_is_segment = m->prog.output_is_segment;
  return XV_OK;
}

double xv_model_macs(const xv_model* m, int32_t frames) { return m ? m->prog.Macs(frames) : 0.0; }

size_t xv_model_describe(const xv_model* m, char* buf, size_t n) {
  if (!m) return 0;
  const std::string s = m->prog.Describe();
  if (buf && n) {
    const size_t k = s.size() < n - 1 ? s.size() : n - 1;
    memcpy(buf, s.data(), k);
    buf[k] = 0;
  }
  return s.size() + 1;
}

xv_status xv_model_pack(const xv_model* m, int precision, void* blob, size_t* nbytes) {
  if (!m || !nbytes) return Fail(XV_ERR_ARG, "xv_model_pack: null argument");
  return Guard([&] {
    std::vector<uint8_t> b = xv::PackModelPolicy(m->prog, precision);
    if (blob) {
      if (*nbytes < b.size()) return Fail(XV_ERR_ARG, "xv_model_pack: buffer too small");
      memcpy(blob, b.data(), b.size());
    }
    *nbytes = b.size();
    return XV_OK;
  });
}

xv_status xv_ctx_create(const xv_model* m, int device, int precision, xv_ctx** out) {
  if (!m || !out) return Fail(XV_ERR_ARG, "xv_ctx_create: null argument");
  return Guard([&] {
    std::vector<uint8_t> b = xv::PackModelPolicy(m->prog, precision);
    std::unique_ptr<xv_ctx> c(new xv_ctx);
    c->eng.reset(new xv::Engine(b.data(), b.size(), device));
    *out = c.release();
    return XV_OK;
  });
}

xv_status xv_ctx_create_from_blob(const void* blob, size_t nbytes, int device, xv_ctx** out) {
  if (!blob || !out) return Fail(XV_ERR_ARG, "xv_ctx_create_from_blob: null argument");
  return Guard([&] {
    std::unique_ptr<xv_ctx> c(new xv_ctx);
    c->eng.reset(new xv::Engine((const uint8_t*)blob, nbytes, device));
    *out = c.release();
    return XV_OK;
  });
}

xv_status xv_ctx_create_from_device_blob(const void* blob_dev, size_t nbytes, int device, xv_ctx** out) {
  if (!blob_dev || !out) return Fail(XV_ERR_ARG, "xv_ctx_create_from_device_blob: null argument");
  return Guard([&] {
    if (hipSetDevice(device) != hipSuccess) return Fail(XV_ERR_DEVICE, "xv_ctx_create_from_device_blob: bad device");
    // header + layer table come back to the host (a few KB); the weights stay on the device
    std::vector<uint8_t> head = xv::ReadBlobHead(blob_dev, nbytes);
    std::unique_ptr<xv_ctx> c(new xv_ctx);
    c->eng.reset(new xv::Engine(head.data(), nbytes, device, blob_dev));
    *out = c.release();
    return XV_OK;
  });
}

void xv_ctx_free(xv_ctx* c) { delete c; }

xv_status xv_ctx_info(const xv_ctx* c, xv_model_info_t* info, int32_t* precision, int32_t* device) {
  if (!c) return Fail(XV_ERR_ARG, "xv_ctx_info: null context");
  if (info) FillInfo(c->eng->info(), info);
  if (precision) *precision = c->eng->info().precision;
  if (device) *device = c->eng->device();
  return XV_OK;
}

xv_status xv_forward_batch(xv_ctx* c, const float* feats, const int32_t* row_offsets, int32_t B, float* out) {
  if (!c || !feats || !row_offsets || !out) return Fail(XV_ERR_ARG, "xv_forward_batch: null argument");
  return Guard([&] {
    for (int b = 0; b < B; ++b)
      if (row_offsets[b + 1] - row_offsets[b] < (c->eng->frame_mode() ? 1 : c->eng->info().min_frames))
        return Fail(XV_ERR_ARG, "xv_forward_batch: chunk " + std::to_string(b) + " has fewer than min_frames rows");
    c->eng->ForwardHost(feats, row_offsets, B, out);
    return XV_OK;
  });
}

xv_status xv_forward_batch_device(xv_ctx* c, const float* feats_dev, const int32_t* row_offsets, int32_t B,
                                  float* out_dev, int32_t out_ld, void* hip_stream) {
  if (!c || !feats_dev || !row_offsets || !out_dev) return Fail(XV_ERR_ARG, "xv_forward_batch_device: null argument");
  return Guard([&] {
    for (int b = 0; b < B; ++b)
      if (row_offsets[b + 1] - row_offsets[b] < (c->eng->frame_mode() ? 1 : c->eng->info().min_frames))
        return Fail(XV_ERR_ARG, "xv_forward_batch_device: chunk " + std::to_string(b) + " has fewer than min_frames rows");
    if (out_ld < c->eng->info().output_dim) return Fail(XV_ERR_ARG, "xv_forward_batch_device: out_ld < output_dim");
    std::shared_ptr<xv::Engine::Plan> plan = c->eng->MakePlan(row_offsets, B);
    c->eng->Forward(*plan, feats_dev, out_dev, out_ld, (hipStream_t)hip_stream);
    return XV_OK;
  });
}

xv_status xv_ctx_synchronize(xv_ctx* c) {
  if (!c) return Fail(XV_ERR_ARG, "xv_ctx_synchronize: null context");
  return Guard([&] {
    if (hipSetDevice(c->eng->device()) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      return Fail(XV_ERR_DEVICE, "hipDeviceSynchronize failed");
    c->eng->CheckKernelFaults();
    return XV_OK;
  });
}

static void FillCalibration(const xv::Engine::Calibration& c, xv_calibration* out) {
  if (!out) return;
  out->chosen = c.chosen;
  out->checked = c.checked;
  out->err_mx = c.err_mx;
  out->err_mx2 = c.err_mx2;
  out->checked_mx = c.checked_mx;
  out->err_lite = c.err_lite;
  out->lite_mask = c.lite_mask;
  out->err_holdout = c.err_holdout;
  out->checked_holdout = c.checked_holdout;
  out->lite_dropped = c.lite_dropped;
  out->tail = c.tail;
}

xv_status xv_ctx_calibrate(xv_ctx* c, const float* feats, const int32_t* row_offsets, int32_t B, float tol, xv_calibration* out) {
  if (!c || !feats || !row_offsets || B < 1) return Fail(XV_ERR_ARG, "xv_ctx_calibrate: bad argument");
  return Guard([&] {
    FillCalibration(c->eng->Calibrate(feats, row_offsets, B, tol), out);
    return XV_OK;
  });
}

xv_status xv_ctx_set_fast_mode(xv_ctx* c, int32_t precision) {
  if (!c) return Fail(XV_ERR_ARG, "xv_ctx_set_fast_mode: null context");
  return Guard([&] {
    if (precision == c->eng->fast_mode() && c->eng->lite_mask() == 0) return XV_OK;
    if (!c->eng->can_switch_fast_mode() || (precision != XV_PREC_FP16MX2 && precision != XV_PREC_FP16MX && precision != XV_PREC_FP16X3))
      return Fail(XV_ERR_ARG, "xv_ctx_set_fast_mode: the context must be packed as XV_PREC_FP16MX2 (pooled output) and the mode one of "
                              "XV_PREC_FP16MX2, XV_PREC_FP16MX, XV_PREC_FP16X3");
    c->eng->SetFastMode(precision);
    return XV_OK;
  });
}

xv_status xv_ctx_fast_mode(const xv_ctx* c, int32_t* precision) {
  if (!c || !precision) return Fail(XV_ERR_ARG, "xv_ctx_fast_mode: null argument");
  *precision = c->eng->fast_mode();
  return XV_OK;
}

xv_status xv_ctx_set_lite_layers(xv_ctx* c, uint64_t mask) {
  if (!c) return Fail(XV_ERR_ARG, "xv_ctx_set_lite_layers: null context");
  return Guard([&] {
    if (mask == c->eng->lite_mask()) return XV_OK;
    if (!c->eng->can_switch_fast_mode() || c->eng->fast_mode() != XV_PREC_FP16MX2)
      return Fail(XV_ERR_ARG, "xv_ctx_set_lite_layers: the context must be running XV_PREC_FP16MX2");
    c->eng->SetLiteMask(mask);
    return XV_OK;
  });
}

xv_status xv_ctx_lite_layers(const xv_ctx* c, uint64_t* mask) {
  if (!c || !mask) return Fail(XV_ERR_ARG, "xv_ctx_lite_layers: null argument");
  *mask = c->eng->lite_mask();
  return XV_OK;
}

xv_status xv_calibrate_table(xv_ctx* c, const char* feature_rspecifier, int32_t chunk_size, int32_t min_chunk_size, int32_t pad_input,
                             int32_t max_utts, float tol, xv_calibration* out) {
  if (!c || !feature_rspecifier) return Fail(XV_ERR_ARG, "xv_calibrate_table: null argument");
  return Guard([&] {
    xv::ExtractOptions opt;
    opt.chunk_size = chunk_size;
    opt.min_chunk_size = min_chunk_size;
    opt.pad_input = pad_input != 0;
    opt.calibrate_tol = tol;
    if (max_utts > 0) opt.calibrate_utts = max_utts;
    if (getenv("XVEC_CMN_WINDOW")) opt.cmn_window = atoi(getenv("XVEC_CMN_WINDOW"));
    if (getenv("XVEC_VAD_RSPECIFIER")) opt.vad_rspecifier = getenv("XVEC_VAD_RSPECIFIER");
    FillCalibration(xv::CalibrateOnTable(c->eng.get(), opt, feature_rspecifier,
                                         [](const char* level, const std::string& m) {
                                           fprintf(stderr, "%s (xvec_hip:xv_calibrate_table) %s\n", level, m.c_str());
                                         }),
                    out);
    return XV_OK;
  });
}

xv_status xv_ctx_set_calibration(xv_ctx* c, int32_t enable, float tol) {
  if (!c) return Fail(XV_ERR_ARG, "xv_ctx_set_calibration: null context");
  c->calibrate = enable != 0;
  if (tol > 0.f) c->calibrate_tol = tol;
  return XV_OK;
}

xv_status xv_ctx_set_calibration_file(xv_ctx* c, const char* path) {
  if (!c) return Fail(XV_ERR_ARG, "xv_ctx_set_calibration_file: null context");
  c->calibration_file = path ? path : "";
  return XV_OK;
}

xv_status xv_recognize_feature_pipeline(const char* rspecifier, int32_t* found, char* feats, size_t feats_cap, char* vad, size_t vad_cap,
                                        int32_t* cmn_window, int32_t* min_cmn_window, int32_t* center) {
  if (!rspecifier || !found) return Fail(XV_ERR_ARG, "xv_recognize_feature_pipeline: null argument");
  return Guard([&] {
    xv::FusedPipeline p;
    *found = xv::RecognizeFeaturePipeline(rspecifier, &p) ? 1 : 0;
    if (*found) {
      if ((feats && p.feats_rspecifier.size() + 1 > feats_cap) || (vad && p.vad_rspecifier.size() + 1 > vad_cap))
        return Fail(XV_ERR_ARG, "xv_recognize_feature_pipeline: output buffer too small");
      if (feats) memcpy(feats, p.feats_rspecifier.c_str(), p.feats_rspecifier.size() + 1);
      if (vad) memcpy(vad, p.vad_rspecifier.c_str(), p.vad_rspecifier.size() + 1);
      if (cmn_window) *cmn_window = p.cmn_window;
      if (min_cmn_window) *min_cmn_window = p.min_cmn_window;
      if (center) *center = p.center ? 1 : 0;
    }
    return XV_OK;
  });
}

xv_status xv_calibration_file_read(const char* path, int32_t* found, uint64_t* model, int32_t* precision, uint64_t* lite_mask) {
  if (!path || !*path || !found) return Fail(XV_ERR_ARG, "xv_calibration_file_read: null argument");
  return Guard([&] {
    xv::SharedChoice sc;
    *found = xv::ReadCalibrationFile(path, &sc) ? 1 : 0;
    if (*found) {
      if (model) *model = sc.model;
      if (precision) *precision = sc.precision;
      if (lite_mask) *lite_mask = sc.lite_mask;
    }
    return XV_OK;
  });
}

xv_status xv_calibration_file_publish(const char* path, uint64_t model, int32_t precision, uint64_t lite_mask, float tol, const char* note,
                                      int32_t* published, uint64_t* adopted_model, int32_t* adopted_precision,
                                      uint64_t* adopted_lite_mask) {
  if (!path || !*path) return Fail(XV_ERR_ARG, "xv_calibration_file_publish: null argument");
  if (precision != XV_PREC_FP16MX && precision != XV_PREC_FP16MX2 && precision != XV_PREC_FP16X3)
    return Fail(XV_ERR_ARG, "xv_calibration_file_publish: the arithmetic must be one of XV_PREC_FP16MX, XV_PREC_FP16MX2, XV_PREC_FP16X3");
  if (lite_mask && precision != XV_PREC_FP16MX2)
    return Fail(XV_ERR_ARG, "xv_calibration_file_publish: lite layers go with XV_PREC_FP16MX2 only");
  return Guard([&] {
    xv::SharedChoice mine, got;
    mine.model = model;
    mine.precision = precision;
    mine.lite_mask = lite_mask;
    mine.tolerance = tol;
    mine.note = note ? note : "";
    for (char& ch : mine.note)
      if (ch == '\n' || ch == '\r') ch = ' ';
    const bool won = xv::PublishCalibrationFile(path, mine, &got);
    if (published) *published = won ? 1 : 0;
    if (adopted_model) *adopted_model = got.model;
    if (adopted_precision) *adopted_precision = got.precision;
    if (adopted_lite_mask) *adopted_lite_mask = got.lite_mask;
    return XV_OK;
  });
}

xv_status xv_ctx_model_fingerprint(const xv_ctx* c, uint64_t* fingerprint) {
  if (!c || !fingerprint) return Fail(XV_ERR_ARG, "xv_ctx_model_fingerprint: null argument");
  *fingerprint = c->eng->info().fingerprint;
  return XV_OK;
}

xv_status xv_ctx_share_calibration(xv_ctx* c, const char* path, float tol, const char* note, int32_t* outcome) {
  if (!c || !path || !*path) return Fail(XV_ERR_ARG, "xv_ctx_share_calibration: null argument");
  return Guard([&] {
    xv::SharedChoice sc;
    int how = 0;
    if (!xv::ReadCalibrationFile(path, &sc)) {
      xv::SharedChoice mine;
      mine.model = c->eng->info().fingerprint;
      mine.precision = c->eng->fast_mode();
      mine.lite_mask = c->eng->lite_mask();
      mine.tolerance = tol;
      mine.note = note ? note : "";
      for (char& ch : mine.note)
        if (ch == '\n' || ch == '\r') ch = ' ';
      how = xv::PublishCalibrationFile(path, mine, &sc) ? 1 : 2;
    }
    xv::AdoptSharedChoice(c->eng.get(), sc, path);
    if (outcome) *outcome = how;
    return XV_OK;
  });
}

xv_status xv_ctx_set_profiling(xv_ctx* c, int32_t enable) {
  if (!c) return Fail(XV_ERR_ARG, "xv_ctx_set_profiling: null context");
  c->eng->SetProfiling(enable != 0);
  return XV_OK;
}

size_t xv_ctx_profile_report(xv_ctx* c, char* buf, size_t n) {
  if (!c) return 0;
  std::string s;
  if (Guard([&] {
        s = c->eng->ProfileReport();
        return XV_OK;
      }) != XV_OK)
    return 0;
  if (buf && n) {
    const size_t k = s.size() < n - 1 ? s.size() : n - 1;
    memcpy(buf, s.data(), k);
    buf[k] = 0;
  }
  return s.size() + 1;
}

xv_status xv_extract_utterances(xv_ctx* c, const float* feats, const int32_t* row_offsets, int32_t n_utts,
                                int32_t chunk_size, int32_t min_chunk_size, int32_t pad_input, float* out, int32_t* ok) {
  if (!c || !feats || !row_offsets || !out || !ok) return Fail(XV_ERR_ARG, "xv_extract_utterances: null argument");
  return Guard([&] {
    xv::ExtractOptions opt;
    opt.chunk_size = chunk_size;
    opt.min_chunk_size = min_chunk_size;
    opt.pad_input = pad_input != 0;
    xv::ExtractUtterances(c->eng.get(), opt, feats, row_offsets, n_utts, out, ok, nullptr);
    return XV_OK;
  });
}

xv_status xv_extract_table(xv_ctx* c, const char* feature_rspecifier, const char* vector_wspecifier, int32_t chunk_size,
                           int32_t min_chunk_size, int32_t pad_input, int32_t batch_frames, int64_t* num_done,
                           int64_t* num_failed) {
  if (!c || !feature_rspecifier || !vector_wspecifier) return Fail(XV_ERR_ARG, "xv_extract_table: null argument");
  return Guard([&] {
    xv::ExtractOptions opt;
    opt.chunk_size = chunk_size;
    opt.min_chunk_size = min_chunk_size;
    opt.pad_input = pad_input != 0;
    if (batch_frames > 0) opt.max_batch_rows = batch_frames;
    opt.calibrate = c->calibrate;
    opt.calibrate_tol = c->calibrate_tol;
    opt.calibration_file = c->calibration_file;
    if (getenv("XVEC_CMN_WINDOW")) opt.cmn_window = atoi(getenv("XVEC_CMN_WINDOW"));
    if (getenv("XVEC_VAD_RSPECIFIER")) opt.vad_rspecifier = getenv("XVEC_VAD_RSPECIFIER");
    xv::TableExtractResult r = xv::RunTableExtraction(
        c->eng.get(), opt, feature_rspecifier, vector_wspecifier, [](const char* level, const std::string& m) {
          fprintf(stderr, "%s (xvec_hip:xv_extract_table) %s\n", level, m.c_str());
        });
    if (num_done) *num_done = r.num_success;
    if (num_failed) *num_failed = r.num_fail;
    return XV_OK;
  });
}

xv_status xv_frontend_cmvn_select(xv_ctx* c, const float* raw, const int32_t* raw_off, int32_t n_utts, const float* vad,
                                  int32_t cmn_window, int32_t center, float* out, int32_t* out_off) {
  if (!c || !raw || !raw_off || !out || !out_off || n_utts < 0) return Fail(XV_ERR_ARG, "xv_frontend_cmvn_select: bad argument");
  return Guard([&] {
    std::vector<int32_t> sel_row, sel_utt;
    out_off[0] = 0;
    for (int u = 0; u < n_utts; ++u) {
      for (int32_t r = raw_off[u]; r < raw_off[u + 1]; ++r)
        if (!vad || vad[r] != 0.f) {
          sel_row.push_back(r);
          sel_utt.push_back(u);
        }
      out_off[u + 1] = (int32_t)sel_row.size();
    }
    c->eng->FrontEndHost(raw, raw_off, n_utts, sel_row.data(), sel_utt.data(), (int)sel_row.size(), cmn_window, center != 0,
                         100, out);
    return XV_OK;
  });
}

xv_status xv_plan_chunks(int32_t num_rows, int32_t chunk_size, int32_t min_chunk_size, int32_t pad_input,
                         int32_t min_net_frames, int32_t cap, int32_t* start, int32_t* len, int32_t* left_pad,
                         int32_t* right_pad, int32_t* n_chunks) {
  if (!n_chunks) return Fail(XV_ERR_ARG, "xv_plan_chunks: null argument");
  return Guard([&] {
    std::vector<xv::Chunk> ch;
    std::string why;
    *n_chunks = 0;
    if (!xv::PlanChunks(0, num_rows, chunk_size, min_chunk_size, pad_input != 0, min_net_frames, &ch, &why))
      return Fail(XV_ERR_ARG, why);
    *n_chunks = (int32_t)ch.size();
    for (int i = 0; i < (int)ch.size() && i < cap; ++i) {
      if (start) start[i] = ch[i].start;
      if (len) len[i] = ch[i].len;
      if (left_pad) left_pad[i] = ch[i].left_pad;
      if (right_pad) right_pad[i] = ch[i].right_pad;
    }
    return XV_OK;
  });
}

xv_status xv_backend_apply(int device, const float* x, int32_t n, int32_t dim, const float* mean, const float* transform,
                           int32_t t_rows, int32_t t_cols, int32_t normalize, int32_t scaleup, float* out, float* ratio) {
  if (n < 0 || dim < 1 || (n > 0 && (!x || !out)) || (transform && t_rows < 1))
    return Fail(XV_ERR_ARG, "xv_backend_apply: bad argument");
  if (transform && t_cols != dim && t_cols != dim + 1)
    return Fail(XV_ERR_ARG, "Dimension mismatch: input vector has dimension " + std::to_string(dim) + " and transform has " +
                                std::to_string(t_cols) + " columns");
  return Guard([&] {
    xv::BackendOptions o;
    o.mean = mean;
    o.transform = transform;
    o.t_rows = t_rows;
    o.t_cols = t_cols;
    o.normalize = normalize != 0;
    o.scaleup = scaleup != 0;
    xv::BackendApply(device, x, n, dim, o, out, ratio);
    return XV_OK;
  });
}

xv_status xv_segment_mean(int device, const float* x, int32_t n, int32_t dim, const int32_t* seg_off, const int32_t* idx,
                          int32_t n_seg, int32_t acc64, float* out) {
  if (n < 0 || dim < 1 || n_seg < 0 || (n_seg > 0 && (!x || !seg_off || !out)))
    return Fail(XV_ERR_ARG, "xv_segment_mean: bad argument");
  for (int s = 0; s < n_seg; ++s)
    if (seg_off[s + 1] < seg_off[s] || seg_off[s] < 0) return Fail(XV_ERR_ARG, "xv_segment_mean: segment offsets must not decrease");
  if (n_seg > 0 && seg_off[n_seg] > 0 && !idx) return Fail(XV_ERR_ARG, "xv_segment_mean: null index list");
  return Guard([&] {
    xv::SegmentMean(device, x, n, dim, seg_off, idx, n_seg, acc64 != 0, out);
    return XV_OK;
  });
}

xv_status xv_scatter_stats(int device, const float* x, int32_t n, int32_t dim, const int32_t* seg_off, const int32_t* idx,
                           int32_t n_seg, double* s_tot, double* sums, double* s_bet, float* device_ms) {
  if (n < 0 || dim < 1 || n_seg < 0 || !seg_off || (n > 0 && !x)) return Fail(XV_ERR_ARG, "xv_scatter_stats: bad argument");
  if (seg_off[0] != 0) return Fail(XV_ERR_ARG, "xv_scatter_stats: segment offsets must start at 0");
  for (int s = 0; s < n_seg; ++s)
    if (seg_off[s + 1] < seg_off[s]) return Fail(XV_ERR_ARG, "xv_scatter_stats: segment offsets must not decrease");
  if (seg_off[n_seg] > 0 && !idx) return Fail(XV_ERR_ARG, "xv_scatter_stats: null index list");
  for (int i = 0; i < seg_off[n_seg]; ++i)
    if (idx[i] < 0 || idx[i] >= n) return Fail(XV_ERR_ARG, "xv_scatter_stats: row index out of range");
  return Guard([&] {
    xv::ScatterStats(device, x, n, dim, seg_off, idx, n_seg, s_tot, sums, s_bet, device_ms);
    return XV_OK;
  });
}

xv_status xv_plda_transform(int device, const float* x, int32_t n, int32_t dim, const double* transform, const double* offset,
                            const double* psi, const double* num, int32_t normalize, int32_t simple, float* y, double* scale,
                            float* device_ms) {
  if (n < 0 || dim < 1 || !transform || !offset || !psi || (n > 0 && (!x || !num || !y)))
    return Fail(XV_ERR_ARG, "xv_plda_transform: bad argument");
  if (dim > xv::kPldaMaxDim) return Fail(XV_ERR_ARG, "xv_plda_transform: dimension larger than " + std::to_string(xv::kPldaMaxDim));
  return Guard([&] {
    xv::PldaTransform(device, x, n, dim, transform, offset, psi, num, normalize != 0, simple != 0, y, scale, device_ms);
    return XV_OK;
  });
}

xv_status xv_plda_score(int device, const float* u, const double* num_u, int32_t n_u, const float* v, int32_t n_v, int32_t dim,
                        const double* psi, const int32_t* trials, int64_t n_trials, double* scores, float* device_ms) {
  if (n_u < 0 || n_v < 0 || dim < 1 || n_trials < 0 || !psi || (n_trials > 0 && (!u || !num_u || !v || !trials || !scores)))
    return Fail(XV_ERR_ARG, "xv_plda_score: bad argument");
  if (dim > xv::kPldaMaxDim) return Fail(XV_ERR_ARG, "xv_plda_score: dimension larger than " + std::to_string(xv::kPldaMaxDim));
  for (int64_t i = 0; i < n_trials; ++i)
    if (trials[2 * i] < 0 || trials[2 * i] >= n_u || trials[2 * i + 1] < 0 || trials[2 * i + 1] >= n_v)
      return Fail(XV_ERR_ARG, "xv_plda_score: trial " + std::to_string(i) + " indexes a row that does not exist");
  return Guard([&] {
    xv::PldaScore(device, u, num_u, n_u, v, n_v, dim, psi, trials, (long)n_trials, scores, device_ms);
    return XV_OK;
  });
}

xv_status xv_plda_score_dense(int device, const float* u, const double* num_u, int32_t n_u, const float* v, int32_t n_v, int32_t dim,
                              const double* psi, double* scores, float* device_ms) {
  if (n_u < 0 || n_v < 0 || dim < 1 || !psi || (n_u > 0 && (!u || !num_u)) || (n_v > 0 && !v) || (n_u > 0 && n_v > 0 && !scores))
    return Fail(XV_ERR_ARG, "xv_plda_score_dense: bad argument");
  if (dim > xv::kPldaMaxDim) return Fail(XV_ERR_ARG, "xv_plda_score_dense: dimension larger than " + std::to_string(xv::kPldaMaxDim));
  for (int32_t k = 0; k < n_u; ++k)
    if (!(num_u[k] > 0)) return Fail(XV_ERR_ARG, "xv_plda_score_dense: example counts must be positive");
  return Guard([&] {
    xv::PldaScoreDense(device, u, num_u, n_u, v, n_v, dim, psi, scores, device_ms);
    return XV_OK;
  });
}

// XV_ERR_ARG unless 2 <= n <= cols <= kTopnMaxCols
static xv_status CheckTopn(const char* who, int64_t cols, int32_t n) {
  if (cols > xv::kTopnMaxCols)
    return Fail(XV_ERR_ARG, std::string(who) + ": " + std::to_string(cols) + " columns are more than kTopnMaxCols = " +
                                std::to_string(xv::kTopnMaxCols));
  if (cols < 2) return Fail(XV_ERR_ARG, std::string(who) + ": the statistics need at least two columns");
  if (n < 2 || n > cols)
    return Fail(XV_ERR_ARG, std::string(who) + ": N = " + std::to_string(n) + " is out of range [2, " + std::to_string(cols) + "]");
  return XV_OK;
}

xv_status xv_topn_stats(int device, const double* scores, int64_t rows, int32_t cols, int32_t n, double* mean, double* std,
                        float* device_ms) {
  if (rows < 0 || rows > 0x7fffffffll || (rows > 0 && (!scores || !mean || !std))) return Fail(XV_ERR_ARG, "xv_topn_stats: bad argument");
  if (const xv_status st = CheckTopn("xv_topn_stats", cols, n)) return st;
  return Guard([&] {
    xv::TopnStats(device, scores, rows, cols, n, mean, std, device_ms);
    return XV_OK;
  });
}

xv_status xv_plda_cohort_stats(int device, const float* u, const double* num_u, int32_t n_u, const float* v, int32_t n_v, int32_t dim,
                               const double* psi, int32_t by_column, int32_t n, double* mean, double* std, float* device_ms) {
  const int32_t rows = by_column ? n_v : n_u;
  if (n_u < 0 || n_v < 0 || dim < 1 || !psi || (n_u > 0 && (!u || !num_u)) || (n_v > 0 && !v) || (rows > 0 && (!mean || !std)))
    return Fail(XV_ERR_ARG, "xv_plda_cohort_stats: bad argument");
  if (dim > xv::kPldaMaxDim) return Fail(XV_ERR_ARG, "xv_plda_cohort_stats: dimension larger than " + std::to_string(xv::kPldaMaxDim));
  if (const xv_status st = CheckTopn("xv_plda_cohort_stats", by_column ? n_u : n_v, n)) return st;
  for (int32_t k = 0; k < n_u; ++k)
    if (!(num_u[k] > 0)) return Fail(XV_ERR_ARG, "xv_plda_cohort_stats: example counts must be positive");
  return Guard([&] {
    xv::PldaCohortStats(device, u, num_u, n_u, v, n_v, dim, psi, by_column != 0, n, mean, std, device_ms);
    return XV_OK;
  });
}

xv_status xv_plda_dense_plan(int64_t rows, int64_t cols, int32_t dim, int64_t workspace_bytes, int64_t* rows_per_chunk,
                             int64_t* n_chunks, int64_t* chunk_bytes) {
  xv::DensePlan plan;
  std::string why;
  if (!xv::PlanPldaDense(rows, cols, dim, workspace_bytes > 0 ? workspace_bytes : xv::kDenseDefaultWorkspace, &plan, &why))
    return Fail(XV_ERR_ARG, "xv_plda_dense_plan: " + why);
  if (rows_per_chunk) *rows_per_chunk = plan.rows_per_chunk;
  if (n_chunks) *n_chunks = plan.n_chunks;
  if (chunk_bytes) *chunk_bytes = plan.chunk_bytes;
  return XV_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// nnet-am-compute (xvec_hip_nnet2.h)
struct xv_nnet2 {
  std::unique_ptr<xv::Nnet2> net;
};

xv_status xv_nnet2_open(const char* model_rxfilename, xv_nnet2** out) {
  if (!model_rxfilename || !out) return Fail(XV_ERR_ARG, "xv_nnet2_open: bad argument");
  *out = nullptr;
  return Guard([&] {
    std::unique_ptr<xv_nnet2> m(new xv_nnet2);
    m->net.reset(new xv::Nnet2(model_rxfilename));
    *out = m.release();
    return XV_OK;
  });
}

void xv_nnet2_close(xv_nnet2* m) { delete m; }

xv_status xv_nnet2_get_info(const xv_nnet2* m, xv_nnet2_info_t* info) {
  if (!m || !info) return Fail(XV_ERR_ARG, "xv_nnet2_get_info: bad argument");
  const xv::Nnet2Model& mod = m->net->model();
  const xv::Nnet2Dims& d = m->net->dims();
  memset(info, 0, sizeof *info);
  info->num_components = (int32_t)mod.components.size();
  info->num_updatable_components = mod.num_updatable;
  info->left_context = d.left_context;
  info->right_context = d.right_context;
  info->input_dim = d.input_dim;
  info->output_dim = d.output_dim;
  info->softmax_dim = d.softmax_dim;
  info->prior_dim = (int32_t)mod.priors.size();
  info->num_layers = (int32_t)mod.layers.size();
  info->max_plane_cols = d.max_plane_cols;
  info->max_pre_cols = d.max_pre_cols;
  info->halo = d.halo;
  info->parameter_dim = mod.parameter_dim;
  return XV_OK;
}

xv_status xv_nnet2_plan(const xv_nnet2_info_t* info, int64_t rows, int64_t block_rows, int64_t workspace_bytes, int64_t* rows_per_block,
                        int64_t* n_blocks, int64_t* bytes) {
  if (!info) return Fail(XV_ERR_ARG, "xv_nnet2_plan: bad argument");
  xv::Nnet2Dims d;
  d.input_dim = info->input_dim;
  d.output_dim = info->output_dim;
  d.softmax_dim = info->softmax_dim;
  d.left_context = info->left_context;
  d.right_context = info->right_context;
  d.max_plane_cols = info->max_plane_cols;
  d.max_pre_cols = info->max_pre_cols;
  d.halo = info->halo;
  xv::Nnet2BlockPlan plan;
  std::string why;
  if (!xv::Nnet2Plan(d, rows, block_rows, workspace_bytes, &plan, &why)) return Fail(XV_ERR_ARG, "xv_nnet2_plan: " + why);
  if (rows_per_block) *rows_per_block = plan.rows_per_block;
  if (n_blocks) *n_blocks = plan.n_blocks;
  if (bytes) *bytes = plan.bytes;
  return XV_OK;
}

// The stage checks its own arguments (nnet2.cc) and says so with Nnet2ArgError.
static xv_status Nnet2Guard(const std::function<void()>& f) {
  return Guard([&] {
    try {
      f();
    } catch (const xv::Nnet2ArgError& e) {
      return Fail(XV_ERR_ARG, e.what());
    }
    return XV_OK;
  });
}

static xv_status Nnet2ComputeCommon(xv_nnet2* m, int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t flags,
                                    int64_t block_rows, float* out, float* device_ms, float* layer_ms) {
  if (!m) return Fail(XV_ERR_ARG, "xv_nnet2_compute: bad argument");
  return Nnet2Guard([&] { m->net->Compute(device, feats, row_off, n_utts, flags, block_rows, out, device_ms, layer_ms); });
}

xv_status xv_nnet2_compute(xv_nnet2* m, int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t flags,
                           int64_t block_rows, float* out, float* device_ms) {
  return Nnet2ComputeCommon(m, device, feats, row_off, n_utts, flags, block_rows, out, device_ms, nullptr);
}

xv_status xv_nnet2_compute_layers(xv_nnet2* m, int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t flags,
                                  int64_t block_rows, float* out, float* layer_ms) {
  if (!layer_ms) return Fail(XV_ERR_ARG, "xv_nnet2_compute_layers: bad argument");
  return Nnet2ComputeCommon(m, device, feats, row_off, n_utts, flags, block_rows, out, nullptr, layer_ms);
}

xv_status xv_nnet2_kernel_affine(int device, const float* x, int32_t rows, int32_t k, const int32_t* context, int32_t n_ctx, const float* w,
                                 const float* bias, int32_t n, float* out) {
  return Nnet2Guard([&] { xv::Nnet2KernelAffine(device, x, rows, k, context, n_ctx, w, bias, n, out); });
}

xv_status xv_nnet2_kernel_row(int device, const float* pre, int32_t rows, int32_t in_dim, int32_t out_dim, int32_t nonlin, int32_t normalize,
                              uint16_t* hi, uint16_t* lo) {
  return Nnet2Guard([&] { xv::Nnet2KernelRow(device, pre, rows, in_dim, out_dim, nonlin, normalize != 0, hi, lo); });
}

xv_status xv_nnet2_kernel_head(int device, const float* logits, int32_t rows, int32_t n, const int32_t* sizes, int32_t n_groups,
                               const float* priors, int32_t apply_log, float* out) {
  return Nnet2Guard([&] { xv::Nnet2KernelHead(device, logits, rows, n, sizes, n_groups, priors, apply_log != 0, out); });
}

xv_status xv_lda_estimate(int32_t dim, int64_t n, const double* s_tot, const double* s_bet, const float* mean,
                          double total_covariance_factor, double covariance_floor, int32_t lda_dim, float* out, int32_t* n_floored) {
  if (dim < 1 || n < 1 || !s_tot || !s_bet || !mean || !out) return Fail(XV_ERR_ARG, "xv_lda_estimate: bad argument");
  if (lda_dim < 1 || lda_dim > dim)
    return Fail(XV_ERR_ARG, "LDA dimension " + std::to_string(lda_dim) + " is out of range for input dimension " + std::to_string(dim));
  return Guard([&] {
    const int f = xv::LdaFromStats(dim, (long)n, s_tot, s_bet, mean, total_covariance_factor, covariance_floor, lda_dim, out);
    if (n_floored) *n_floored = f;
    return XV_OK;
  });
}

xv_status xv_plda_estimate(int32_t dim, int32_t n_spk, const double* sums, const int32_t* counts, const double* s_tot,
                           const double* s_bet, int32_t num_em_iters, double* mean, double* transform, double* psi,
                           int32_t* n_floored) {
  if (dim < 1 || n_spk < 1 || num_em_iters < 0 || !sums || !counts || !s_tot || !s_bet || !mean || !transform || !psi)
    return Fail(XV_ERR_ARG, "xv_plda_estimate: bad argument");
  for (int k = 0; k < n_spk; ++k)
    if (counts[k] < 1) return Fail(XV_ERR_ARG, "xv_plda_estimate: every speaker needs at least one vector");
  return Guard([&] {
    xv::Plda p;
    const int f = xv::PldaFromStats(dim, n_spk, sums, counts, s_tot, s_bet, num_em_iters, &p);
    std::copy(p.mean.begin(), p.mean.end(), mean);
    std::copy(p.transform.begin(), p.transform.end(), transform);
    std::copy(p.psi.begin(), p.psi.end(), psi);
    if (n_floored) *n_floored = f;
    return XV_OK;
  });
}

xv_status xv_plda_adapt(int32_t dim, int64_t n, const double* m, const double* v, const double* mean, const double* transform,
                        const double* psi, double mean_diff_scale, double within_covar_scale, double between_covar_scale,
                        double* mean_out, double* transform_out, double* psi_out, double* s_out) {
  if (dim < 1 || n < 1 || !m || !v || !mean || !transform || !psi || !mean_out || !transform_out || !psi_out)
    return Fail(XV_ERR_ARG, "xv_plda_adapt: bad argument");
  for (int d = 0; d < dim; ++d)
    if (!(psi[d] >= 0.0)) return Fail(XV_ERR_ARG, "xv_plda_adapt: psi must not be negative");
  return Guard([&] {
    xv::Plda p;
    p.dim = dim;
    p.mean.assign(mean, mean + dim);
    p.transform.assign(transform, transform + (size_t)dim * dim);
    p.psi.assign(psi, psi + dim);
    xv::AdaptPlda((long)n, m, v, mean_diff_scale, within_covar_scale, between_covar_scale, &p, s_out);
    std::copy(p.mean.begin(), p.mean.end(), mean_out);
    std::copy(p.transform.begin(), p.transform.end(), transform_out);
    std::copy(p.psi.begin(), p.psi.end(), psi_out);
    return XV_OK;
  });
}

// Feature stage: feat.cc (tables, device calls), wave.cc (RIFF reader).
void xv_mfcc_options_default(xv_mfcc_options* opts) {
  if (opts) *opts = xv::MfccDefaults();
}

int64_t xv_mfcc_num_frames(const xv_mfcc_options* opts, int64_t n_samples) {
  if (!opts) {
    Fail(XV_ERR_ARG, "xv_mfcc_num_frames: null options");
    return -1;
  }
  try {
    g_err.clear();
    return xv::MfccNumFrames(*opts, n_samples);
  } catch (const std::exception& e) {
    Fail(XV_ERR_ARG, e.what());
    return -1;
  }
}

uint64_t xv_mfcc_utt_seed(const char* key) { return xv::UttSeed(key); }

namespace {
xv_status MfccComputeCommon(int device, const xv_mfcc_options* opts, const void* samples, bool is_i16, const int64_t* sample_offsets,
                            int32_t n_utts, const uint64_t* utt_seeds, float* out, int32_t* out_row_offsets) {
  if (!opts || !sample_offsets || !out_row_offsets || n_utts < 0) return Fail(XV_ERR_ARG, "xv_mfcc_compute: bad argument");
  for (int u = 0; u < n_utts; ++u)
    if (sample_offsets[u + 1] < sample_offsets[u] || sample_offsets[u] < 0)
      return Fail(XV_ERR_ARG, "xv_mfcc_compute: sample offsets must not decrease");
  if (n_utts > 0 && sample_offsets[n_utts] > sample_offsets[0] && !samples) return Fail(XV_ERR_ARG, "xv_mfcc_compute: null samples");
  if (opts->dither != 0.f && !utt_seeds && n_utts > 0)
    return Fail(XV_ERR_ARG, "xv_mfcc_compute: dither != 0 needs utt_seeds (xv_mfcc_utt_seed of each utterance key)");
  try {
    (void)xv::MfccGeometryOf(*opts);
    (void)xv::BuildMfccTables(*opts);
  } catch (const std::exception& e) {
    return Fail(XV_ERR_ARG, e.what());
  }
  return Guard([&] {
    xv::MfccComputer mc(device, *opts);
    std::vector<float> feats;
    mc.Compute(samples, is_i16, sample_offsets, n_utts, utt_seeds, &feats, out_row_offsets);
    if (!feats.empty()) {
      if (!out) return Fail(XV_ERR_ARG, "xv_mfcc_compute: null output");
      memcpy(out, feats.data(), feats.size() * sizeof(float));
    }
    return XV_OK;
  });
}
}  // namespace

xv_status xv_mfcc_compute(int device, const xv_mfcc_options* opts, const float* samples, const int64_t* sample_offsets,
                          int32_t n_utts, const uint64_t* utt_seeds, float* out, int32_t* out_row_offsets) {
  return MfccComputeCommon(device, opts, samples, false, sample_offsets, n_utts, utt_seeds, out, out_row_offsets);
}

xv_status xv_mfcc_compute_i16(int device, const xv_mfcc_options* opts, const int16_t* samples, const int64_t* sample_offsets,
                              int32_t n_utts, const uint64_t* utt_seeds, float* out, int32_t* out_row_offsets) {
  return MfccComputeCommon(device, opts, samples, true, sample_offsets, n_utts, utt_seeds, out, out_row_offsets);
}

xv_status xv_mfcc_kernel_time(int device, const xv_mfcc_options* opts, const int16_t* samples, const int64_t* sample_offsets,
                              int32_t n_utts, int32_t reps, float* kernel_ms) {
  if (!opts || !samples || !sample_offsets || !kernel_ms || n_utts < 1 || reps < 1) return Fail(XV_ERR_ARG, "xv_mfcc_kernel_time: bad argument");
  return Guard([&] {
    xv::MfccComputer mc(device, *opts);
    std::vector<float> feats;
    std::vector<int32_t> row_off(n_utts + 1);
    std::vector<uint64_t> seeds(n_utts, 1);
    xv::BestOfReps(reps, 1, kernel_ms, [&](int, float* ms) {
      mc.Compute(samples, true, sample_offsets, n_utts, seeds.data(), &feats, row_off.data(), ms);
    });
    return XV_OK;
  });
}

xv_status xv_vad_energy(int device, const xv_vad_options* vad_opts, const float* feats, const int32_t* row_offsets,
                        int32_t n_utts, int32_t dim, float* out) {
  if (!vad_opts || !row_offsets || n_utts < 0 || dim < 1) return Fail(XV_ERR_ARG, "xv_vad_energy: bad argument");
  if (n_utts > 0 && row_offsets[n_utts] > 0 && (!feats || !out)) return Fail(XV_ERR_ARG, "xv_vad_energy: null buffer");
  if (vad_opts->vad_frames_context < 0 || !(vad_opts->vad_proportion_threshold > 0.f && vad_opts->vad_proportion_threshold < 1.f))
    return Fail(XV_ERR_ARG, "xv_vad_energy: vad_frames_context must be >= 0 and vad_proportion_threshold in (0, 1)");
  return Guard([&] {
    xv::VadEnergy(device, *vad_opts, feats, row_offsets, n_utts, dim, out);
    return XV_OK;
  });
}

xv_status xv_wave_read(const char* rxfilename, int32_t channel, int32_t* rate, int16_t** samples, int64_t* n) {
  if (!rxfilename || !rate || !samples || !n) return Fail(XV_ERR_ARG, "xv_wave_read: null argument");
  *samples = nullptr;
  *n = 0;
  return Guard([&] {
    xv::Input in;
    in.Open(rxfilename);
    xv::WaveData w;
    xv::ReadWave(in, &w, true);
    std::vector<int16_t> one;
    xv::SelectChannel(w, channel, &one, nullptr);
    int16_t* p = (int16_t*)malloc(one.size() * 2 + 2);
    if (!p) throw std::bad_alloc();
    memcpy(p, one.data(), one.size() * 2);
    *samples = p;
    *n = (int64_t)one.size();
    *rate = w.rate;
    return XV_OK;
  });
}

void xv_wave_free(int16_t* samples) { free(samples); }

xv_status xv_wave_write(const char* wxfilename, int32_t rate, const float* samples, int64_t n, int64_t* clipped) {
  if (!wxfilename || n < 0 || (n > 0 && !samples)) return Fail(XV_ERR_ARG, "xv_wave_write: bad argument");
  return Guard([&] {
    const int64_t c = xv::WriteWave(wxfilename, rate, samples, n);
    if (clipped) *clipped = c;
    return XV_OK;
  });
}

xv_status xv_recognize_cmvn_pipeline(const char* rspecifier, int32_t* found, char* description, size_t description_cap) {
  if (!rspecifier || !found) return Fail(XV_ERR_ARG, "xv_recognize_cmvn_pipeline: null argument");
  return Guard([&] {
    xv::FusedCmvnPipeline p;
    *found = xv::RecognizeCmvnPipeline(rspecifier, &p) ? 1 : 0;
    if (*found && description) {
      const std::string d = xv::DescribeFusedCmvn(p);
      if (d.size() + 1 > description_cap) return Fail(XV_ERR_ARG, "xv_recognize_cmvn_pipeline: output buffer too small");
      memcpy(description, d.c_str(), d.size() + 1);
    }
    return XV_OK;
  });
}

xv_status xv_recognize_wav_pipeline(const char* rxfilename, int32_t* found, char* description, size_t description_cap) {
  if (!rxfilename || !found) return Fail(XV_ERR_ARG, "xv_recognize_wav_pipeline: null argument");
  return Guard([&] {
    xv::FusedWav p;
    *found = xv::RecognizeWavPipeline(rxfilename, &p) ? 1 : 0;
    if (*found && description) {
      const std::string d = xv::DescribeFusedWav(p);
      if (d.size() + 1 > description_cap) return Fail(XV_ERR_ARG, "xv_recognize_wav_pipeline: output buffer too small");
      memcpy(description, d.c_str(), d.size() + 1);
    }
    return XV_OK;
  });
}

void xv_reverb_options_default(xv_reverb_options* opts) {
  if (opts) *opts = xv::ReverbDefaults();
}

int64_t xv_reverb_output_length(const xv_reverb_options* opts, float sample_rate, int64_t n_samples, int64_t rir_len) {
  if (!opts) {
    Fail(XV_ERR_ARG, "xv_reverb_output_length: null options");
    return -1;
  }
  return xv::ReverbOutputLength(*opts, sample_rate, n_samples, rir_len);
}

namespace {
void FillReverbBatch(xv::ReverbBatch* out, float sample_rate, const void* samples, int32_t samples_are_i16, const int64_t* sample_offsets,
                              int32_t n_utts, const float* rirs, const int64_t* rir_offsets, int32_t n_rirs, const int32_t* utt_rir,
                              const float* noises, const int64_t* noise_offsets, int32_t n_noises, const int32_t* utt_add_offsets,
                              const int32_t* add_noise, const float* add_snr, const float* add_start) {
  xv::ReverbBatch b;
  b.rate = sample_rate;
  b.samples = samples;
  b.is_i16 = samples_are_i16 != 0;
  b.sample_off = sample_offsets;
  b.n_utts = n_utts;
  b.rirs = rirs;
  b.rir_off = rir_offsets;
  b.n_rirs = n_rirs;
  b.utt_rir = n_rirs > 0 ? utt_rir : nullptr;
  b.noises = noises;
  b.noise_off = noise_offsets;
  b.n_noises = n_noises;
  b.utt_add_off = utt_add_offsets;
  b.add_noise = add_noise;
  b.add_snr = add_snr;
  b.add_start = add_start;
  *out = b;
}
}  // namespace

xv_status xv_wav_reverberate(int device, const xv_reverb_options* opts, float sample_rate, const void* samples,
                             int32_t samples_are_i16, const int64_t* sample_offsets, int32_t n_utts, const float* rirs,
                             const int64_t* rir_offsets, int32_t n_rirs, const int32_t* utt_rir, const float* noises,
                             const int64_t* noise_offsets, int32_t n_noises, const int32_t* utt_add_offsets,
                             const int32_t* add_noise, const float* add_snr, const float* add_start, int64_t* out_offsets,
                             float* out_f32, int16_t* out_i16, int64_t* clipped) {
  if (!opts || !sample_offsets || !out_offsets || n_utts < 0) return Fail(XV_ERR_ARG, "xv_wav_reverberate: bad argument");
  if (utt_add_offsets && n_utts > 0 && utt_add_offsets[n_utts] > utt_add_offsets[0] && (!add_noise || !add_snr || !add_start))
    return Fail(XV_ERR_ARG, "xv_wav_reverberate: additive signals without their index, SNR or start time");
  return Guard([&] {
    xv::ReverbBatch b;
    FillReverbBatch(&b, sample_rate, samples, samples_are_i16, sample_offsets, n_utts, rirs, rir_offsets, n_rirs,
                                            utt_rir, noises, noise_offsets, n_noises, utt_add_offsets, add_noise, add_snr, add_start);
    xv::Reverberate(device, *opts, b, out_offsets, out_f32, out_i16, clipped);
    return XV_OK;
  });
}

xv_status xv_reverb_kernel_time(int device, const xv_reverb_options* opts, float sample_rate, const void* samples,
                                int32_t samples_are_i16, const int64_t* sample_offsets, int32_t n_utts, const float* rirs,
                                const int64_t* rir_offsets, int32_t n_rirs, const int32_t* utt_rir, const float* noises,
                                const int64_t* noise_offsets, int32_t n_noises, const int32_t* utt_add_offsets,
                                const int32_t* add_noise, const float* add_snr, const float* add_start, int32_t reps,
                                float* kernel_ms) {
  if (!opts || !sample_offsets || !kernel_ms || n_utts < 1 || reps < 1) return Fail(XV_ERR_ARG, "xv_reverb_kernel_time: bad argument");
  return Guard([&] {
    xv::ReverbBatch b;
    FillReverbBatch(&b, sample_rate, samples, samples_are_i16, sample_offsets, n_utts, rirs, rir_offsets, n_rirs,
                                            utt_rir, noises, noise_offsets, n_noises, utt_add_offsets, add_noise, add_snr, add_start);
    std::vector<int64_t> off(n_utts + 1);
    int64_t total = 0;
    for (int u = 0; u < n_utts; ++u) {
      const int ri = b.utt_rir ? b.utt_rir[u] : -1;
      const int64_t rl = ri >= 0 && ri < n_rirs ? rir_offsets[ri + 1] - rir_offsets[ri] : 0;
      total += std::max<int64_t>(0, xv::ReverbOutputLength(*opts, sample_rate, sample_offsets[u + 1] - sample_offsets[u], rl));
    }
    std::vector<float> out((size_t)total + 1);
    xv::BestOfReps(reps, 1, kernel_ms, [&](int, float* ms) {
      xv::Reverberate(device, *opts, b, off.data(), out.data(), nullptr, nullptr, ms);
    });
    return XV_OK;
  });
}

// Compressed feature matrices and the model-free sliding CMN: compress.cc.
xv_status xv_compressed_size(int32_t rows, int32_t cols, int32_t method, size_t* nbytes, const char** format) {
  if (rows < 0 || cols < 0) return Fail(XV_ERR_ARG, "xv_compressed_size: bad argument");
  if (!xv::CompressedSize(rows, cols, method, nbytes, format)) return Fail(XV_ERR_ARG, xv::CompressionMethodError(method));
  g_err.clear();
  return XV_OK;
}

xv_status xv_compress_matrices(int device, const float* feats, const int32_t* row_off, int32_t n, int32_t cols, int32_t method,
                               uint8_t* out_bytes, int64_t* out_off, int32_t* nonfinite_flags) {
  if (n < 0 || cols < 0 || !row_off || !out_off) return Fail(XV_ERR_ARG, "xv_compress_matrices: bad argument");
  if (!xv::CompressionMethodError(method).empty()) return Fail(XV_ERR_ARG, xv::CompressionMethodError(method));
  return Guard([&] {
    xv::CompressMatrices(device, feats, row_off, n, cols, method, out_bytes, out_off, nonfinite_flags);
    return XV_OK;
  });
}

xv_status xv_compress_kernel_time(int device, const float* feats, const int32_t* row_off, int32_t n, int32_t cols, int32_t method,
                                  int32_t reps, float* kernel_ms) {
  if (!feats || !row_off || !kernel_ms || n < 1 || cols < 1 || reps < 1) return Fail(XV_ERR_ARG, "xv_compress_kernel_time: bad argument");
  if (!xv::CompressionMethodError(method).empty()) return Fail(XV_ERR_ARG, xv::CompressionMethodError(method));
  return Guard([&] {
    std::vector<int64_t> off(n + 1);
    size_t total = 0;
    for (int u = 0; u < n; ++u) {
      size_t nb = 0;
      xv::CompressedSize(row_off[u + 1] - row_off[u], cols, method, &nb, nullptr);
      total += nb;
    }
    std::vector<uint8_t> out(total + 1);
    xv::BestOfReps(reps, 1, kernel_ms, [&](int, float* ms) {
      xv::CompressMatrices(device, feats, row_off, n, cols, method, out.data(), off.data(), nullptr, ms);
    });
    return XV_OK;
  });
}

xv_status xv_cmvn_sliding(int device, const float* raw, const int32_t* raw_off, int32_t n, int32_t cols, int32_t cmn_window,
                          int32_t min_cmn_window, int32_t center, float* out) {
  if (n < 0 || cols < 1 || !raw_off) return Fail(XV_ERR_ARG, "xv_cmvn_sliding: bad argument");
  return Guard([&] {
    xv::CmvnSliding(device, raw, raw_off, n, cols, cmn_window, min_cmn_window, center != 0, out);
    return XV_OK;
  });
}

xv_status xv_cmvn_stats(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, double* stats,
                        float* device_ms) {
  if (n_utts < 0 || cols < 1 || !row_off || (n_utts > 0 && !stats)) return Fail(XV_ERR_ARG, "xv_cmvn_stats: bad argument");
  return Guard([&] {
    xv::CmvnStats(device, feats, row_off, n_utts, cols, stats, device_ms);
    return XV_OK;
  });
}

xv_status xv_cmvn_norm(const double* stats, int32_t cols, int32_t norm_means, int32_t norm_vars, int32_t reverse,
                       const int32_t* skip_dims, int32_t n_skip, float* norm, int32_t* num_floored) {
  return Guard([&] {
    try {
      const int floored = xv::CmvnNorm(stats, cols, norm_means != 0, norm_vars != 0, reverse != 0, skip_dims, n_skip, norm);
      if (num_floored) *num_floored = floored;
    } catch (const xv::CmvnArgError& e) {
      return Fail(XV_ERR_ARG, e.what());
    }
    return XV_OK;
  });
}

xv_status xv_cmvn_apply(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, const float* norms,
                        const int32_t* utt_norm, float* out) {
  if (n_utts < 0 || cols < 1 || !row_off || (n_utts > 0 && (!utt_norm || !norms))) return Fail(XV_ERR_ARG, "xv_cmvn_apply: bad argument");
  int n_norms = 0;
  for (int u = 0; u < n_utts; ++u) {
    if (utt_norm[u] < 0) return Fail(XV_ERR_ARG, "xv_cmvn_apply: negative norm index");
    n_norms = utt_norm[u] + 1 > n_norms ? utt_norm[u] + 1 : n_norms;
  }
  return Guard([&] {
    xv::CmvnApply(device, feats, row_off, n_utts, cols, norms, n_norms, utt_norm, out);
    return XV_OK;
  });
}

xv_status xv_cmvn_apply_select(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, const float* norms,
                               int32_t n_norms, const int32_t* utt_norm, const int32_t* sel_row, const int32_t* sel_utt, int32_t n_out,
                               float* out) {
  if (n_utts < 0 || cols < 1 || !row_off || n_norms < 0 || n_out < 0) return Fail(XV_ERR_ARG, "xv_cmvn_apply_select: bad argument");
  return Guard([&] {
    xv::CmvnApplySelect(device, feats, row_off, n_utts, cols, norms, n_norms, utt_norm, sel_row, sel_utt, n_out, out);
    return XV_OK;
  });
}

xv_status xv_cmvn_kernel_time(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, int32_t reps,
                              float* stats_ms, float* apply_ms) {
  if (!feats || !row_off || !stats_ms || !apply_ms || n_utts < 1 || cols < 1 || reps < 1)
    return Fail(XV_ERR_ARG, "xv_cmvn_kernel_time: bad argument");
  return Guard([&] {
    std::vector<double> stats((size_t)n_utts * 2 * (cols + 1));
    std::vector<float> norms((size_t)n_utts * 2 * cols), out((size_t)row_off[n_utts] * cols);
    std::vector<int32_t> utt_norm(n_utts);
    float best[2];
    xv::BestOfReps(reps, 2, best, [&](int r, float* ms) {
      xv::CmvnStats(device, feats, row_off, n_utts, cols, stats.data(), &ms[0]);
      if (r == 0)
        for (int u = 0; u < n_utts; ++u) {
          utt_norm[u] = u;
          xv::CmvnNorm(stats.data() + (size_t)u * 2 * (cols + 1), cols, true, true, false, nullptr, 0, norms.data() + (size_t)u * 2 * cols);
        }
      xv::CmvnApply(device, feats, row_off, n_utts, cols, norms.data(), n_utts, utt_norm.data(), out.data(), &ms[1]);
    });
    *stats_ms = best[0];
    *apply_ms = best[1];
    return XV_OK;
  });
}

struct xv_ubm {
  std::unique_ptr<xv::UbmModel> m;
};

xv_status xv_add_deltas(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, int32_t order,
                        int32_t window, int32_t truncate, float* out, float* device_ms) {
  if (n_utts < 0 || cols < 1 || !row_off) return Fail(XV_ERR_ARG, "xv_add_deltas: bad argument");
  return Guard([&] {
    xv::AddDeltas(device, feats, row_off, n_utts, cols, order, window, truncate, out, device_ms);
    return XV_OK;
  });
}

xv_status xv_ubm_diag_create(int device, int32_t num_gauss, int32_t dim, const float* gconsts, const float* means_invvars,
                             const float* inv_vars, xv_ubm** out) {
  if (!out) return Fail(XV_ERR_ARG, "xv_ubm_diag_create: bad argument");
  return Guard([&] {
    std::unique_ptr<xv_ubm> h(new xv_ubm);
    h->m.reset(xv::UbmDiagCreate(device, num_gauss, dim, gconsts, means_invvars, inv_vars));
    *out = h.release();
    return XV_OK;
  });
}

xv_status xv_ubm_full_create(int device, int32_t num_gauss, int32_t dim, const float* gconsts, const float* means_invcovars,
                             const float* inv_covars, xv_ubm** out) {
  if (!out) return Fail(XV_ERR_ARG, "xv_ubm_full_create: bad argument");
  return Guard([&] {
    std::unique_ptr<xv_ubm> h(new xv_ubm);
    h->m.reset(xv::UbmFullCreate(device, num_gauss, dim, gconsts, means_invcovars, inv_covars));
    *out = h.release();
    return XV_OK;
  });
}

void xv_ubm_destroy(xv_ubm* m) { delete m; }

xv_status xv_ubm_gselect(const xv_ubm* diag, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t n, int32_t* idx,
                         float* loglikes, float* device_ms) {
  if (!diag || !row_off || n_utts < 0) return Fail(XV_ERR_ARG, "xv_ubm_gselect: bad argument");
  return Guard([&] {
    xv::UbmGselect(*diag->m, feats, row_off, n_utts, n, idx, loglikes, device_ms);
    return XV_OK;
  });
}

xv_status xv_ubm_post(const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* gselect, int32_t n,
                      float min_post, int32_t* count, int32_t* idx, float* post, float* loglikes, float* logsum, float* device_ms3) {
  if (!full || !row_off || n_utts < 0) return Fail(XV_ERR_ARG, "xv_ubm_post: bad argument");
  return Guard([&] {
    xv::UbmPost(*full->m, feats, row_off, n_utts, gselect, n, min_post, count, idx, post, loglikes, logsum, device_ms3);
    return XV_OK;
  });
}

xv_status xv_fgmm_to_gmm(int32_t num_gauss, int32_t dim, const float* weights, const float* means_invcovars, const float* inv_covars,
                         float* gconsts_out, float* means_invvars_out, float* inv_vars_out) {
  if (num_gauss < 1 || dim < 1 || !weights || !means_invcovars || !inv_covars || !gconsts_out || !means_invvars_out || !inv_vars_out)
    return Fail(XV_ERR_ARG, "xv_fgmm_to_gmm: bad argument");
  return Guard([&] {
    xv::FullGmmData f;
    f.num_gauss = num_gauss;
    f.dim = dim;
    f.weights.assign(weights, weights + num_gauss);
    f.means_invcovars.assign(means_invcovars, means_invcovars + (size_t)num_gauss * dim);
    f.inv_covars.assign(inv_covars, inv_covars + (size_t)num_gauss * ((size_t)dim * (dim + 1) / 2));
    xv::DiagGmmData d;
    xv::FullGmmToDiag(f, &d);
    std::copy(d.gconsts.begin(), d.gconsts.end(), gconsts_out);
    std::copy(d.means_invvars.begin(), d.means_invvars.end(), means_invvars_out);
    std::copy(d.inv_vars.begin(), d.inv_vars.end(), inv_vars_out);
    return XV_OK;
  });
}

xv_status xv_fgmm_gconsts(int32_t num_gauss, int32_t dim, const float* weights, const float* means_invcovars, const float* inv_covars,
                          float* gconsts_out, int32_t* num_bad) {
  if (num_gauss < 1 || dim < 1 || !weights || !means_invcovars || !inv_covars || !gconsts_out) return Fail(XV_ERR_ARG, "xv_fgmm_gconsts: bad argument");
  return Guard([&] {
    xv::FullGmmData f;
    f.num_gauss = num_gauss;
    f.dim = dim;
    f.weights.assign(weights, weights + num_gauss);
    f.means_invcovars.assign(means_invcovars, means_invcovars + (size_t)num_gauss * dim);
    f.inv_covars.assign(inv_covars, inv_covars + (size_t)num_gauss * ((size_t)dim * (dim + 1) / 2));
    const int bad = xv::ComputeGconsts(&f);
    if (num_bad) *num_bad = bad;
    std::copy(f.gconsts.begin(), f.gconsts.end(), gconsts_out);
    return XV_OK;
  });
}

xv_status xv_ubm_kernel_time(const xv_ubm* diag, const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts,
                             int32_t n, float min_post, int32_t reps, float* ms5) {
  if (!diag || !full || !feats || !row_off || n_utts < 1 || reps < 1 || !ms5) return Fail(XV_ERR_ARG, "xv_ubm_kernel_time: bad argument");
  if (diag->m->full() || !full->m->full() || diag->m->dim() != full->m->dim() || diag->m->device() != full->m->device())
    return Fail(XV_ERR_ARG, "xv_ubm_kernel_time: a diagonal and a full model of one dimension on one device");
  if (n < 1 || n > 64 || n > diag->m->num_gauss() || row_off[0] != 0 || row_off[n_utts] < 1)
    return Fail(XV_ERR_ARG, "xv_ubm_kernel_time: 1 <= n <= min(64, the model's size) and at least one frame");
  return Guard([&] {
    const size_t rows = (size_t)row_off[n_utts];
    const int dim = diag->m->dim();
    std::vector<int32_t> gs(rows * n), count(rows), idx(rows * n);
    std::vector<float> post(rows * n), deltas(dim % 3 == 0 ? rows * dim : 0);
    xv::BestOfReps(reps, 5, ms5, [&](int, float* ms) {
      if (dim % 3 == 0) xv::AddDeltas(diag->m->device(), feats, row_off, n_utts, dim, 2, 3, dim / 3, deltas.data(), &ms[0]);
      xv::UbmGselect(*diag->m, feats, row_off, n_utts, n, gs.data(), nullptr, &ms[1]);
      xv::UbmPost(*full->m, feats, row_off, n_utts, gs.data(), n, min_post, count.data(), idx.data(), post.data(), nullptr, nullptr, &ms[2]);
    });
    return XV_OK;
  });
}

xv_status xv_ubm_full_gselect(const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* preselect,
                              int32_t n_in, int32_t n_out, int32_t* idx, float* loglikes, float* device_ms3) {
  if (!full || !row_off || n_utts < 0) return Fail(XV_ERR_ARG, "xv_ubm_full_gselect: bad argument");
  return Guard([&] {
    xv::UbmFullGselect(*full->m, feats, row_off, n_utts, preselect, n_in, n_out, idx, loglikes, device_ms3);
    return XV_OK;
  });
}

xv_status xv_ubm_frame_likes(const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* gselect, int32_t n,
                             float* likes, float* device_ms3) {
  if (!full || !row_off || n_utts < 0) return Fail(XV_ERR_ARG, "xv_ubm_frame_likes: bad argument");
  return Guard([&] {
    xv::UbmFrameLikes(*full->m, feats, row_off, n_utts, gselect, n, likes, device_ms3);
    return XV_OK;
  });
}

xv_status xv_vad_from_frame_likes(int32_t n_classes, const float* const* likes, int64_t rows, const float* priors, const int32_t* map, float* out) {
  return Guard([&] {
    xv::VadFromFrameLikes(n_classes, likes, rows, priors, map, out);
    return XV_OK;
  });
}

xv_status xv_merge_vads(const float* a, const float* b, int64_t rows, const int32_t* map_triples, int32_t n_triples, float* out) {
  return Guard([&] {
    xv::MergeVads(a, b, rows, map_triples, n_triples, out);
    return XV_OK;
  });
}

struct xv_fgmm_acc {
  std::unique_ptr<xv::FgmmAccumulator> a;
};

xv_status xv_fgmm_acc_create(int device, int32_t num_gauss, int32_t dim, const char* update_flags, xv_fgmm_acc** out) {
  if (!out || !update_flags) return Fail(XV_ERR_ARG, "xv_fgmm_acc_create: bad argument");
  return Guard([&] {
    std::unique_ptr<xv_fgmm_acc> h(new xv_fgmm_acc);
    h->a.reset(xv::FgmmAccCreate(device, num_gauss, dim, xv::ParseGmmFlags(update_flags)));
    *out = h.release();
    return XV_OK;
  });
}

void xv_fgmm_acc_destroy(xv_fgmm_acc* a) { delete a; }

xv_status xv_fgmm_acc_add(xv_fgmm_acc* a, const float* feats, int32_t rows, const int32_t* post_off, const int32_t* post_idx,
                          const float* post_w) {
  if (!a || rows < 0 || !post_off) return Fail(XV_ERR_ARG, "xv_fgmm_acc_add: bad argument");
  return Guard([&] {
    xv::FgmmAccAdd(a->a.get(), feats, rows, post_off, post_idx, post_w);
    return XV_OK;
  });
}

xv_status xv_fgmm_acc_add_gselect(xv_fgmm_acc* a, const xv_ubm* full, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  float* logsum) {
  if (!a || !full || rows < 0) return Fail(XV_ERR_ARG, "xv_fgmm_acc_add_gselect: bad argument");
  return Guard([&] {
    xv::FgmmAccAddGselect(a->a.get(), *full->m, feats, rows, gselect, n, logsum);
    return XV_OK;
  });
}

xv_status xv_fgmm_acc_get(const xv_fgmm_acc* a, double* occ, double* mean, double* cov) {
  if (!a) return Fail(XV_ERR_ARG, "xv_fgmm_acc_get: bad argument");
  return Guard([&] {
    xv::FgmmAccGet(*a->a, occ, mean, cov);
    return XV_OK;
  });
}

namespace {

// the caller's arrays into accumulators of either kind; `second` (named by second_name in the error) is cov or var
void FillGmmAccs(const char* who, const char* second_name, int32_t num_gauss, int32_t dim, const char* acc_flags, const double* occ, const double* mean,
                 const double* second, xv::GmmAccs* accs) {
  accs->Init(num_gauss, dim, xv::ParseGmmFlags(acc_flags));
  std::copy(occ, occ + num_gauss, accs->occ.begin());
  if (accs->flags & xv::kFgmmFlagMeans) {
    if (!mean) throw xv::KioError(std::string(who) + ": the flags ask for mean accumulators");
    std::copy(mean, mean + (size_t)num_gauss * dim, accs->mean.begin());
  }
  if (accs->flags & xv::kFgmmFlagVariances) {
    if (!second) throw xv::KioError(std::string(who) + ": the flags ask for " + second_name + " accumulators");
    std::copy(second, second + (size_t)num_gauss * accs->second_width(), accs->second.begin());
  }
}

void CopyGmmEstResult(const xv::GmmEstResult& r, int32_t* floored2, double* objf3) {
  if (floored2) {
    floored2[0] = r.floored_elements;
    floored2[1] = r.floored_gauss;
  }
  if (objf3) {
    objf3[0] = r.objf_before;
    objf3[1] = r.objf_after;
    objf3[2] = r.count;
  }
}

}  // namespace

xv_status xv_fgmm_est(int32_t num_gauss, int32_t dim, const char* acc_flags, const double* occ, const double* mean, const double* cov,
                      const char* update_flags, double min_gaussian_weight, double min_gaussian_occupancy, double variance_floor,
                      double max_condition, int32_t remove_low_count_gaussians, float* weights, float* means_invcovars, float* inv_covars,
                      float* gconsts, int32_t* num_gauss_out, int32_t* removed, int32_t* floored2, double* objf3) {
  if (num_gauss < 1 || dim < 1 || !acc_flags || !occ || !update_flags || !weights || !means_invcovars || !inv_covars || !gconsts || !num_gauss_out)
    return Fail(XV_ERR_ARG, "xv_fgmm_est: bad argument");
  return Guard([&] {
    const size_t tri = (size_t)dim * (dim + 1) / 2;
    xv::FgmmAccs accs;
    FillGmmAccs("xv_fgmm_est", "covariance", num_gauss, dim, acc_flags, occ, mean, cov, &accs);
    xv::FullGmmData m;
    m.num_gauss = num_gauss;
    m.dim = dim;
    m.weights.assign(weights, weights + num_gauss);
    m.means_invcovars.assign(means_invcovars, means_invcovars + (size_t)num_gauss * dim);
    m.inv_covars.assign(inv_covars, inv_covars + (size_t)num_gauss * tri);
    xv::ComputeGconsts(&m);
    xv::FgmmEstOptions o;
    o.min_gaussian_weight = min_gaussian_weight;
    o.min_gaussian_occupancy = min_gaussian_occupancy;
    o.variance_floor = variance_floor;
    o.max_condition = max_condition;
    o.remove_low_count_gaussians = remove_low_count_gaussians != 0;
    xv::FgmmEstResult r;
    xv::FgmmEst(accs, xv::ParseGmmFlags(update_flags), o, &m, &r);
    std::copy(m.weights.begin(), m.weights.end(), weights);
    std::copy(m.means_invcovars.begin(), m.means_invcovars.end(), means_invcovars);
    std::copy(m.inv_covars.begin(), m.inv_covars.end(), inv_covars);
    std::copy(m.gconsts.begin(), m.gconsts.end(), gconsts);
    *num_gauss_out = m.num_gauss;
    if (removed) std::copy(r.removed.begin(), r.removed.end(), removed);
    CopyGmmEstResult(r, floored2, objf3);
    return XV_OK;
  });
}

xv_status xv_fgmm_acc_kernel_time(xv_fgmm_acc* a, const xv_ubm* full, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  int32_t reps, float* ms4) {
  if (!a || !full || !feats || !gselect || rows < 1 || reps < 1 || !ms4) return Fail(XV_ERR_ARG, "xv_fgmm_acc_kernel_time: bad argument");
  return Guard([&] {
    std::vector<float> logsum((size_t)rows);
    xv::BestOfReps(reps, 4, ms4, [&](int, float* ms) {
      xv::FgmmAccAddGselect(a->a.get(), *full->m, feats, rows, gselect, n, logsum.data(), ms);
    });
    return XV_OK;
  });
}

xv_status xv_logprob_to_post(int device, const float* logprobs, const int32_t* row_off, int32_t n_utts, int32_t cols, const char* const* keys,
                             float min_post, int32_t random_prune, int32_t frame_budget, int64_t capacity, int64_t* pair_off, int32_t* idx,
                             float* post, int64_t* need, int64_t* num_nan, float* device_ms3) {
  if (!row_off || n_utts < 0 || !pair_off || !need || capacity < 0 || (capacity > 0 && (!idx || !post)))
    return Fail(XV_ERR_ARG, "xv_logprob_to_post: bad argument");
  return Guard([&] {
    std::vector<uint64_t> seeds;
    if (keys)
      for (int32_t u = 0; u < n_utts; ++u) {
        if (!keys[u]) return Fail(XV_ERR_ARG, "xv_logprob_to_post: null key");
        seeds.push_back(xv::UttSeed(keys[u]));
      }
    xv::LogprobPostResult r;
    xv::LogprobToPost(device, logprobs, row_off, n_utts, cols, keys ? seeds.data() : nullptr, min_post, random_prune != 0, frame_budget,
                      device_ms3 != nullptr, &r);
    std::copy(r.off.begin(), r.off.end(), pair_off);
    *need = r.off.back();
    if (num_nan) *num_nan = r.num_nan;
    if (device_ms3) std::copy(r.ms, r.ms + 3, device_ms3);
    if (*need <= capacity) {
      std::copy(r.idx.begin(), r.idx.end(), idx);
      std::copy(r.w.begin(), r.w.end(), post);
    }
    return XV_OK;
  });
}

xv_status xv_logprob_to_post_kernel_time(int device, const float* logprobs, int32_t rows, int32_t cols, const char* key, float min_post,
                                         int32_t random_prune, int32_t reps, float* ms4) {
  if (!logprobs || rows < 1 || cols < 1 || !key || reps < 1 || !ms4) return Fail(XV_ERR_ARG, "xv_logprob_to_post_kernel_time: bad argument");
  if ((int64_t)rows * cols > INT32_MAX) return Fail(XV_ERR_ARG, "xv_logprob_to_post_kernel_time: rows * cols must fit one launch (below 2^31)");
  return Guard([&] {
    const int32_t row_off[2] = {0, rows};
    const uint64_t seed = xv::UttSeed(key);
    xv::BestOfReps(reps, 3, ms4, [&](int, float* ms) {
      xv::LogprobPostResult res;
      xv::LogprobToPost(device, logprobs, row_off, 1, cols, &seed, min_post, random_prune != 0, rows, true, &res);
      std::copy(res.ms, res.ms + 3, ms);
    });
    ms4[3] = xv::DeviceCopyMs(device, (size_t)rows * cols * 4, reps);
    return XV_OK;
  });
}

xv_status xv_fgmm_init_from_accs(int32_t num_gauss, int32_t dim, const double* occ, const double* mean, const double* cov,
                                 int32_t remove_low_count_gaussians, float* weights_out, float* means_invcovars_out, float* inv_covars_out,
                                 float* gconsts_out, int32_t* num_gauss_out, int32_t* removed, int32_t* num_bad_gconsts, double* inv_covars_f64) {
  if (num_gauss < 1 || dim < 1 || !occ || !mean || !cov || !weights_out || !means_invcovars_out || !inv_covars_out || !gconsts_out || !num_gauss_out)
    return Fail(XV_ERR_ARG, "xv_fgmm_init_from_accs: bad argument");
  return Guard([&] {
    xv::FgmmAccs accs;
    FillGmmAccs("xv_fgmm_init_from_accs", "covariance", num_gauss, dim, "mvw", occ, mean, cov, &accs);
    xv::FullGmmData m;
    xv::FgmmInitResult r;
    xv::FgmmInitFromAccs(accs, remove_low_count_gaussians != 0, &m, &r);
    std::copy(m.weights.begin(), m.weights.end(), weights_out);
    std::copy(m.means_invcovars.begin(), m.means_invcovars.end(), means_invcovars_out);
    std::copy(m.inv_covars.begin(), m.inv_covars.end(), inv_covars_out);
    std::copy(m.gconsts.begin(), m.gconsts.end(), gconsts_out);
    *num_gauss_out = m.num_gauss;
    if (removed) std::copy(r.removed.begin(), r.removed.end(), removed);
    if (num_bad_gconsts) *num_bad_gconsts = r.bad_gconsts;
    if (inv_covars_f64) std::copy(r.inv_covars64.begin(), r.inv_covars64.end(), inv_covars_f64);
    return XV_OK;
  });
}

struct xv_dgmm_acc {
  std::unique_ptr<xv::DgmmAccumulator> a;
};

xv_status xv_dgmm_acc_create(int device, int32_t num_gauss, int32_t dim, const char* update_flags, xv_dgmm_acc** out) {
  if (!out || !update_flags) return Fail(XV_ERR_ARG, "xv_dgmm_acc_create: bad argument");
  return Guard([&] {
    std::unique_ptr<xv_dgmm_acc> h(new xv_dgmm_acc);
    h->a.reset(xv::DgmmAccCreate(device, num_gauss, dim, xv::ParseGmmFlags(update_flags)));
    *out = h.release();
    return XV_OK;
  });
}

void xv_dgmm_acc_destroy(xv_dgmm_acc* a) { delete a; }

xv_status xv_dgmm_acc_add(xv_dgmm_acc* a, const float* feats, int32_t rows, const int32_t* post_off, const int32_t* post_idx,
                          const float* post_w) {
  if (!a || rows < 0 || !post_off) return Fail(XV_ERR_ARG, "xv_dgmm_acc_add: bad argument");
  return Guard([&] {
    xv::DgmmAccAdd(a->a.get(), feats, rows, post_off, post_idx, post_w);
    return XV_OK;
  });
}

xv_status xv_dgmm_acc_add_gselect(xv_dgmm_acc* a, const xv_ubm* diag, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  float* loglikes, float* logsum) {
  if (!a || !diag || rows < 0) return Fail(XV_ERR_ARG, "xv_dgmm_acc_add_gselect: bad argument");
  return Guard([&] {
    xv::DgmmAccAddGselect(a->a.get(), *diag->m, feats, rows, gselect, n, loglikes, logsum);
    return XV_OK;
  });
}

xv_status xv_dgmm_acc_add_dense_post(xv_dgmm_acc* a, const float* feats, int32_t rows, const float* post) {
  if (!a || rows < 0) return Fail(XV_ERR_ARG, "xv_dgmm_acc_add_dense_post: bad argument");
  return Guard([&] {
    xv::DgmmAccAddDensePost(a->a.get(), feats, rows, post);
    return XV_OK;
  });
}

xv_status xv_dgmm_acc_add_dense(xv_dgmm_acc* a, const xv_ubm* diag, const float* feats, int32_t rows, float* logsum) {
  if (!a || !diag || rows < 0 || (rows > 0 && !feats)) return Fail(XV_ERR_ARG, "xv_dgmm_acc_add_dense: bad argument");
  return Guard([&] {
    xv::DgmmAccAddDense(a->a.get(), *diag->m, feats, rows, logsum);
    return XV_OK;
  });
}

xv_status xv_dgmm_acc_get(const xv_dgmm_acc* a, double* occ, double* mean, double* var) {
  if (!a) return Fail(XV_ERR_ARG, "xv_dgmm_acc_get: bad argument");
  return Guard([&] {
    xv::DgmmAccGet(*a->a, occ, mean, var);
    return XV_OK;
  });
}

xv_status xv_dgmm_est(int32_t num_gauss, int32_t dim, const char* acc_flags, const double* occ, const double* mean, const double* var,
                      const char* update_flags, double min_gaussian_weight, double min_gaussian_occupancy, double min_variance,
                      int32_t remove_low_count_gaussians, int32_t mix_up, double perturb_factor, uint64_t seed, float* weights,
                      float* means_invvars, float* inv_vars, float* gconsts, int32_t* num_gauss_out, int32_t* removed, int32_t* num_removed,
                      int32_t* floored2, double* objf3, int32_t* split_of) {
  if (num_gauss < 1 || dim < 1 || !acc_flags || !occ || !update_flags || !weights || !means_invvars || !inv_vars || !gconsts || !num_gauss_out)
    return Fail(XV_ERR_ARG, "xv_dgmm_est: bad argument");
  return Guard([&] {
    xv::DgmmAccs accs;
    FillGmmAccs("xv_dgmm_est", "variance", num_gauss, dim, acc_flags, occ, mean, var, &accs);
    xv::DiagGmmData m;
    m.num_gauss = num_gauss;
    m.dim = dim;
    m.weights.assign(weights, weights + num_gauss);
    m.means_invvars.assign(means_invvars, means_invvars + (size_t)num_gauss * dim);
    m.inv_vars.assign(inv_vars, inv_vars + (size_t)num_gauss * dim);
    xv::ComputeGconsts(&m);
    xv::DgmmEstOptions o;
    o.min_gaussian_weight = min_gaussian_weight;
    o.min_gaussian_occupancy = min_gaussian_occupancy;
    o.min_variance = min_variance;
    o.remove_low_count_gaussians = remove_low_count_gaussians != 0;
    xv::DgmmEstResult r;
    xv::DgmmEst(accs, xv::ParseGmmFlags(update_flags), o, &m, &r);
    std::vector<int32_t> from;
    xv::DgmmSplit(&m, mix_up, perturb_factor, seed, 0, &from);
    std::copy(m.weights.begin(), m.weights.end(), weights);
    std::copy(m.means_invvars.begin(), m.means_invvars.end(), means_invvars);
    std::copy(m.inv_vars.begin(), m.inv_vars.end(), inv_vars);
    std::copy(m.gconsts.begin(), m.gconsts.end(), gconsts);
    *num_gauss_out = m.num_gauss;
    if (removed) std::copy(r.removed.begin(), r.removed.end(), removed);
    if (num_removed) *num_removed = (int32_t)r.removed.size();
    if (split_of) std::copy(from.begin(), from.end(), split_of);
    CopyGmmEstResult(r, floored2, objf3);
    return XV_OK;
  });
}

xv_status xv_dgmm_acc_kernel_time(xv_dgmm_acc* a, const xv_ubm* diag, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  int32_t dense, int32_t reps, float* ms7) {
  if (!a || !diag || !feats || rows < 1 || reps < 1 || !ms7) return Fail(XV_ERR_ARG, "xv_dgmm_acc_kernel_time: bad argument");
  return Guard([&] {
    std::vector<float> logsum((size_t)rows);
    xv::BestOfReps(reps, 7, ms7, [&](int, float* ms) {
      if (gselect) xv::DgmmAccAddGselect(a->a.get(), *diag->m, feats, rows, gselect, n, nullptr, logsum.data(), ms);
      if (dense) xv::DgmmAccAddDense(a->a.get(), *diag->m, feats, rows, logsum.data(), ms + 4);
    });
    return XV_OK;
  });
}

struct xv_ivex {
  std::unique_ptr<xv::IvexModel> m;
};

namespace {

void FillIvexData(int32_t G, int32_t D, int32_t S, const double* w_vec, const double* M, const double* sigma_inv, double prior_offset, xv::IvexData* d) {
  if (G < 1 || D < 1 || S < 1 || !w_vec || !M || !sigma_inv) throw xv::KioError("i-vector extractor: bad argument");
  d->G = G;
  d->D = D;
  d->S = S;
  d->w_vec.assign(w_vec, w_vec + G);
  d->M.assign(M, M + (size_t)G * D * S);
  d->sigma_inv.assign(sigma_inv, sigma_inv + (size_t)G * ((size_t)D * (D + 1) / 2));
  d->prior_offset = prior_offset;
}

}  // namespace

xv_status xv_ivex_create(int device, int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, const double* w_vec, const double* M,
                         const double* sigma_inv, double prior_offset, xv_ivex** out) {
  if (!out) return Fail(XV_ERR_ARG, "xv_ivex_create: bad argument");
  return Guard([&] {
    xv::IvexData d;
    FillIvexData(num_gauss, feat_dim, ivector_dim, w_vec, M, sigma_inv, prior_offset, &d);
    std::unique_ptr<xv_ivex> h(new xv_ivex);
    h->m.reset(xv::IvexCreate(device, d));
    *out = h.release();
    return XV_OK;
  });
}

xv_status xv_ivex_load(int device, const char* rxfilename, xv_ivex** out) {
  if (!out || !rxfilename) return Fail(XV_ERR_ARG, "xv_ivex_load: bad argument");
  return Guard([&] {
    xv::IvexData d;
    xv::ReadIvexFile(rxfilename, &d);
    std::unique_ptr<xv_ivex> h(new xv_ivex);
    h->m.reset(xv::IvexCreate(device, d));
    *out = h.release();
    return XV_OK;
  });
}

void xv_ivex_destroy(xv_ivex* m) { delete m; }

xv_status xv_ivex_info(const xv_ivex* m, int32_t* num_gauss, int32_t* feat_dim, int32_t* ivector_dim) {
  if (!m) return Fail(XV_ERR_ARG, "xv_ivex_info: bad argument");
  if (num_gauss) *num_gauss = m->m->num_gauss();
  if (feat_dim) *feat_dim = m->m->feat_dim();
  if (ivector_dim) *ivector_dim = m->m->ivector_dim();
  return XV_OK;
}

xv_status xv_ivex_derived(const xv_ivex* m, double* sigma_inv_m, double* U) {
  if (!m) return Fail(XV_ERR_ARG, "xv_ivex_derived: bad argument");
  return Guard([&] {
    xv::IvexDerived(*m->m, sigma_inv_m, U);
    return XV_OK;
  });
}

xv_status xv_ivex_extract(xv_ivex* m, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off,
                          const int32_t* post_idx, const float* post_w, double acoustic_weight, double max_count, float* ivectors,
                          int32_t* status, double* auxf_change, double* gamma, double* X, double* linear, double* quadratic) {
  if (!m || !row_off || n_utts < 0) return Fail(XV_ERR_ARG, "xv_ivex_extract: bad argument");
  return Guard([&] {
    xv::IvexOutputs o;
    o.ivectors = ivectors;
    o.status = status;
    o.auxf_change = auxf_change;
    o.gamma = gamma;
    o.X = X;
    o.linear = linear;
    o.quadratic = quadratic;
    xv::IvexExtract(*m->m, feats, row_off, n_utts, post_off, post_idx, post_w, acoustic_weight, max_count, o);
    return XV_OK;
  });
}

xv_status xv_ivex_read(const char* rxfilename, int32_t* num_gauss, int32_t* feat_dim, int32_t* ivector_dim, double* w_vec, double* M,
                       double* sigma_inv, double* prior_offset) {
  if (!rxfilename) return Fail(XV_ERR_ARG, "xv_ivex_read: bad argument");
  return Guard([&] {
    xv::IvexData d;
    xv::ReadIvexFile(rxfilename, &d);
    if (num_gauss) *num_gauss = d.G;
    if (feat_dim) *feat_dim = d.D;
    if (ivector_dim) *ivector_dim = d.S;
    if (w_vec) std::copy(d.w_vec.begin(), d.w_vec.end(), w_vec);
    if (M) std::copy(d.M.begin(), d.M.end(), M);
    if (sigma_inv) std::copy(d.sigma_inv.begin(), d.sigma_inv.end(), sigma_inv);
    if (prior_offset) *prior_offset = d.prior_offset;
    return XV_OK;
  });
}

xv_status xv_ivex_write(const char* wxfilename, int32_t binary, int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, const double* w_vec,
                        const double* M, const double* sigma_inv, double prior_offset) {
  if (!wxfilename) return Fail(XV_ERR_ARG, "xv_ivex_write: bad argument");
  return Guard([&] {
    xv::IvexData d;
    FillIvexData(num_gauss, feat_dim, ivector_dim, w_vec, M, sigma_inv, prior_offset, &d);
    xv::WriteIvexFile(wxfilename, binary != 0, d);
    return XV_OK;
  });
}

xv_status xv_ivex_kernel_time(xv_ivex* m, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off,
                              const int32_t* post_idx, const float* post_w, int32_t reps, float* ms5) {
  if (!m || !feats || !row_off || !post_off || n_utts < 1 || reps < 1 || !ms5) return Fail(XV_ERR_ARG, "xv_ivex_kernel_time: bad argument");
  return Guard([&] {
    const int S = m->m->ivector_dim();
    std::vector<float> iv((size_t)n_utts * S);
    std::vector<int32_t> status((size_t)n_utts);
    std::vector<double> auxf((size_t)n_utts);
    xv::BestOfReps(reps, 4, ms5, [&](int, float* ms) {
      xv::IvexOutputs o;
      o.ivectors = iv.data();
      o.status = status.data();
      o.auxf_change = auxf.data();
      o.device_ms4 = ms;
      xv::IvexExtract(*m->m, feats, row_off, n_utts, post_off, post_idx, post_w, 1.0, 0.0, o);
    });
    ms5[4] = m->m->derive_ms();
    return XV_OK;
  });
}

// ---- i-vector extractor training (ivex_train.h)
struct xv_ivex_acc {
  std::unique_ptr<xv::IvexAccumulator> a;
};

namespace {

size_t TriOf(int32_t d) { return (size_t)d * (d + 1) / 2; }

void FillIvexStats(int32_t G, int32_t D, int32_t S, int32_t has_variances, const double* scalars3, const double* gamma, const double* Y, const double* R,
                   const double* Sg, const double* ivector_sum, const double* ivector_scatter, xv::IvexStats* st) {
  if (!scalars3 || !gamma || !Y || !R || !ivector_sum || !ivector_scatter || (has_variances && !Sg)) throw xv::KioError("i-vector extractor statistics: null array");
  st->Init(G, D, S, has_variances != 0);
  st->num_ivectors = scalars3[0];
  st->auxf = scalars3[1];
  st->frames = scalars3[2];
  std::copy(gamma, gamma + st->gamma.size(), st->gamma.begin());
  std::copy(Y, Y + st->Y.size(), st->Y.begin());
  std::copy(R, R + st->R.size(), st->R.begin());
  if (has_variances) std::copy(Sg, Sg + st->Sg.size(), st->Sg.begin());
  std::copy(ivector_sum, ivector_sum + st->ivector_sum.size(), st->ivector_sum.begin());
  std::copy(ivector_scatter, ivector_scatter + st->ivector_scatter.size(), st->ivector_scatter.begin());
}

void CopyIvexStats(const xv::IvexStats& st, double* scalars3, double* gamma, double* Y, double* R, double* Sg, double* ivector_sum, double* ivector_scatter) {
  if (scalars3) {
    scalars3[0] = st.num_ivectors;
    scalars3[1] = st.auxf;
    scalars3[2] = st.frames;
  }
  if (gamma) std::copy(st.gamma.begin(), st.gamma.end(), gamma);
  if (Y) std::copy(st.Y.begin(), st.Y.end(), Y);
  if (R) std::copy(st.R.begin(), st.R.end(), R);
  if (Sg) std::copy(st.Sg.begin(), st.Sg.end(), Sg);
  if (ivector_sum) std::copy(st.ivector_sum.begin(), st.ivector_sum.end(), ivector_sum);
  if (ivector_scatter) std::copy(st.ivector_scatter.begin(), st.ivector_scatter.end(), ivector_scatter);
}

}  // namespace

xv_status xv_ivex_acc_create(const xv_ivex* m, int32_t update_variances, int32_t compute_auxf, xv_ivex_acc** out) {
  if (!m || !out) return Fail(XV_ERR_ARG, "xv_ivex_acc_create: bad argument");
  return Guard([&] {
    std::unique_ptr<xv_ivex_acc> h(new xv_ivex_acc);
    h->a.reset(xv::IvexAccCreate(m->m.get(), update_variances != 0, compute_auxf != 0));
    *out = h.release();
    return XV_OK;
  });
}

void xv_ivex_acc_destroy(xv_ivex_acc* a) { delete a; }

xv_status xv_ivex_acc_add(xv_ivex_acc* a, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off, const int32_t* post_idx,
                          const float* post_w, int32_t* status) {
  if (!a || !row_off || n_utts < 0) return Fail(XV_ERR_ARG, "xv_ivex_acc_add: bad argument");
  return Guard([&] {
    xv::IvexAccAdd(a->a.get(), feats, row_off, n_utts, post_off, post_idx, post_w, status);
    return XV_OK;
  });
}

xv_status xv_ivex_acc_get(xv_ivex_acc* a, double* scalars3, double* gamma, double* Y, double* R, double* Sg, double* ivector_sum,
                          double* ivector_scatter) {
  if (!a) return Fail(XV_ERR_ARG, "xv_ivex_acc_get: bad argument");
  return Guard([&] {
    xv::IvexStats st;
    xv::IvexAccGet(a->a.get(), &st);
    CopyIvexStats(st, scalars3, gamma, Y, R, st.has_variances ? Sg : nullptr, ivector_sum, ivector_scatter);
    return XV_OK;
  });
}

xv_status xv_ivex_acc_pending(xv_ivex_acc* a, int32_t* count, double* m, double* scatter, double* logdet, double* auxf) {
  if (!a || !count) return Fail(XV_ERR_ARG, "xv_ivex_acc_pending: bad argument");
  return Guard([&] {
    *count = xv::IvexAccPending(a->a.get(), m, scatter, logdet, auxf);
    return XV_OK;
  });
}

xv_status xv_ivex_acc_kernel_time(xv_ivex_acc* a, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off,
                                  const int32_t* post_idx, const float* post_w, int32_t reps, float* ms3) {
  if (!a || !feats || !row_off || !post_off || n_utts < 1 || reps < 1 || !ms3) return Fail(XV_ERR_ARG, "xv_ivex_acc_kernel_time: bad argument");
  return Guard([&] {
    xv::IvexStats st;
    xv::BestOfReps(reps, 3, ms3, [&](int, float* ms) {
      float add[3], get[3];
      xv::IvexAccAdd(a->a.get(), feats, row_off, n_utts, post_off, post_idx, post_w, nullptr, add);
      xv::IvexAccGet(a->a.get(), &st, get);
      for (int i = 0; i < 3; ++i) ms[i] = add[i] + get[i];
    });
    return XV_OK;
  });
}

xv_status xv_ivex_rank_update(int device, const double* A, const double* B, double* C, int32_t slots, int64_t M, int64_t N, int64_t c_rows, int64_t ldc) {
  return Guard([&] {
    xv::IvexRankUpdateHost(device, A, B, C, slots, M, N, c_rows, ldc);
    return XV_OK;
  });
}

xv_status xv_ivex_init(int32_t num_gauss, int32_t feat_dim, const float* weights, const float* means_invcovars, const float* inv_covars,
                       int32_t ivector_dim, uint64_t seed, double* w_vec, double* M, double* sigma_inv, double* prior_offset) {
  if (num_gauss < 1 || feat_dim < 1 || !weights || !means_invcovars || !inv_covars || !w_vec || !M || !sigma_inv || !prior_offset)
    return Fail(XV_ERR_ARG, "xv_ivex_init: bad argument");
  return Guard([&] {
    xv::FullGmmData ubm;
    ubm.num_gauss = num_gauss;
    ubm.dim = feat_dim;
    ubm.weights.assign(weights, weights + num_gauss);
    ubm.means_invcovars.assign(means_invcovars, means_invcovars + (size_t)num_gauss * feat_dim);
    ubm.inv_covars.assign(inv_covars, inv_covars + (size_t)num_gauss * TriOf(feat_dim));
    xv::IvexData d;
    xv::IvexInit(ubm, ivector_dim, seed, &d);
    std::copy(d.w_vec.begin(), d.w_vec.end(), w_vec);
    std::copy(d.M.begin(), d.M.end(), M);
    std::copy(d.sigma_inv.begin(), d.sigma_inv.end(), sigma_inv);
    *prior_offset = d.prior_offset;
    return XV_OK;
  });
}

xv_status xv_ivex_est(int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, int32_t has_variances, const double* scalars3, const double* gamma,
                      const double* Y, const double* R, const double* Sg, const double* ivector_sum, const double* ivector_scatter,
                      double variance_floor_factor, double gaussian_min_count, int32_t diagonalize, int32_t num_threads, const double* w_vec, double* M,
                      double* sigma_inv, double* prior_offset, int32_t* counts6, double* impr3, double* V) {
  if (!prior_offset) return Fail(XV_ERR_ARG, "xv_ivex_est: bad argument");
  return Guard([&] {
    xv::IvexStats st;
    FillIvexStats(num_gauss, feat_dim, ivector_dim, has_variances, scalars3, gamma, Y, R, Sg, ivector_sum, ivector_scatter, &st);
    xv::IvexData d;
    FillIvexData(num_gauss, feat_dim, ivector_dim, w_vec, M, sigma_inv, *prior_offset, &d);
    xv::IvexEstOptions o;
    o.variance_floor_factor = variance_floor_factor;
    o.gaussian_min_count = gaussian_min_count;
    o.diagonalize = diagonalize != 0;
    o.num_threads = num_threads;
    xv::IvexEstResult r;
    xv::IvexEst(st, o, &d, &r);
    std::copy(d.M.begin(), d.M.end(), M);
    std::copy(d.sigma_inv.begin(), d.sigma_inv.end(), sigma_inv);
    *prior_offset = d.prior_offset;
    if (counts6) {
      counts6[0] = r.gauss_updated;
      counts6[1] = r.gauss_skipped;
      counts6[2] = r.eig_floored;
      counts6[3] = r.var_floored;
      counts6[4] = r.var_floored_gauss;
      counts6[5] = r.prior_floored;
    }
    if (impr3) {
      impr3[0] = r.impr_proj;
      impr3[1] = r.impr_var;
      impr3[2] = r.impr_prior;
    }
    if (V) std::copy(r.V.begin(), r.V.end(), V);
    return XV_OK;
  });
}

xv_status xv_ivex_stats_read(const char* rxfilename, int32_t* num_gauss, int32_t* feat_dim, int32_t* ivector_dim, int32_t* has_variances, double* scalars3,
                             double* gamma, double* Y, double* R, double* Sg, double* ivector_sum, double* ivector_scatter) {
  if (!rxfilename) return Fail(XV_ERR_ARG, "xv_ivex_stats_read: bad argument");
  return Guard([&] {
    xv::IvexStats st;
    xv::ReadIvexStatsFile(rxfilename, &st);
    if (num_gauss) *num_gauss = st.G;
    if (feat_dim) *feat_dim = st.D;
    if (ivector_dim) *ivector_dim = st.S;
    if (has_variances) *has_variances = st.has_variances ? 1 : 0;
    CopyIvexStats(st, scalars3, gamma, Y, R, st.has_variances ? Sg : nullptr, ivector_sum, ivector_scatter);
    return XV_OK;
  });
}

xv_status xv_ivex_stats_write(const char* wxfilename, int32_t binary, int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, int32_t has_variances,
                              const double* scalars3, const double* gamma, const double* Y, const double* R, const double* Sg, const double* ivector_sum,
                              const double* ivector_scatter) {
  if (!wxfilename) return Fail(XV_ERR_ARG, "xv_ivex_stats_write: bad argument");
  return Guard([&] {
    xv::IvexStats st;
    FillIvexStats(num_gauss, feat_dim, ivector_dim, has_variances, scalars3, gamma, Y, R, Sg, ivector_sum, ivector_scatter, &st);
    xv::WriteIvexStatsFile(wxfilename, binary != 0, st);
    return XV_OK;
  });
}

// One process, several GPUs: multi_gpu.cc (one ncclBroadcast of the packed image, bounded wait, contexts from the device copies).
xv_status xv_ctx_create_broadcast(const xv_model* m, const int* devices, int n, int precision, xv_ctx** out) {
  if (!m || !devices || !out || n < 1) return Fail(XV_ERR_ARG, "xv_ctx_create_broadcast: bad argument");
  return Guard([&]() -> xv_status {
    const std::vector<uint8_t> blob = xv::PackModelPolicy(m->prog, precision);
    std::vector<std::unique_ptr<xv::Engine>> engines = xv::CreateEnginesBroadcast(blob, std::vector<int>(devices, devices + n));
    for (int i = 0; i < n; ++i) {
      xv_ctx* c = new xv_ctx;
      c->eng = std::move(engines[i]);
      out[i] = c;
    }
    return XV_OK;
  });
}

// xv_gemm_desc -> GemmArgs, for the launch entry and the plan entry: "" or what is wrong with the descriptor.  Split-K: the slices
// are the engine's rule; splitk_ws is the caller's.
static std::string GemmArgsFromDesc(const xv_gemm_desc* d, xv::GemmArgs* out) {
  if (d->nseg < 1 || d->nseg > xv::kMaxSeg || d->rows % xv::kBM || d->n_pad % xv::kBN) return "bad geometry";
  xv::GemmArgs& a = *out;
  memset(&a, 0, sizeof a);
  a.nseg = d->nseg;
  for (int j = 0; j < d->nseg; ++j) {
    if (d->seg[j].k_len % xv::kBK) return "k_len must be a multiple of 32";
    a.seg[j].hi = (const uint16_t*)d->seg[j].hi;
    a.seg[j].lo = (const uint16_t*)d->seg[j].lo;
    a.seg[j].ld = d->seg[j].ld;
    a.seg[j].row_shift = d->seg[j].row_shift;
    a.seg[j].ksteps = d->seg[j].k_len / xv::kBK;
    a.seg[j].gmax = (const unsigned*)d->seg[j].gmax;
    a.seg[j].lo4 = (const uint8_t*)d->seg[j].lo4;
    a.seg[j].lo4s = (const uint8_t*)d->seg[j].lo4_scale;
    a.total_ksteps += a.seg[j].ksteps;
  }
  a.w_hi = (const uint16_t*)d->w_hi;
  a.w_lo = (const uint16_t*)d->w_lo;
  a.ldw = d->ldw;
  a.m_tiles = d->rows / xv::kBM;
  a.n_tiles = d->n_pad / xv::kBN;
  a.relu = d->relu;
  a.bn = d->bn;
  a.bias = d->bias;
  a.scale = d->scale;
  a.offset = d->offset;
  a.out_hi = (uint16_t*)d->out_hi;
  a.out_lo = (uint16_t*)d->out_lo;
  a.ldo = d->ldo;
  a.out_f32 = d->out_f32;
  a.ldf = d->ldf;
  a.m_valid = d->m_valid;
  a.partial = d->partial;
  a.ldp = d->ldp;
  a.grp_range = d->grp_range;
  a.w4 = (const uint8_t*)d->w4;
  a.ldw4 = d->ldw4;
  a.w4_scale = (const uint8_t*)d->w4_scale;
  a.gmax_out = (unsigned*)d->gmax_out;
  a.w4b = (const uint8_t*)d->w4b;
  a.ldw4b = d->ldw4b;
  a.w4b_scale = (const uint8_t*)d->w4b_scale;
  a.out_lo4 = (uint8_t*)d->out_lo4;
  a.out_lo4s = (uint8_t*)d->out_lo4_scale;
  a.p8 = d->p8;
  a.out_range = d->out_range;
  if (d->ksplit > 1) {
    if (d->precision < xv::kPrecBf16x3 || d->precision > xv::kPrecFp16x3 || a.p8 ||
        (d->epilogue != xv::kEpiAct && d->epilogue != xv::kEpiF32))
      return "split-K needs XV_PREC_BF16X3 .. XV_PREC_FP16X3, epilogue 0 or 1 and no p8";
    a.ksteps_per_slice = xv::SplitKStepsPerSlice(a.total_ksteps);
    a.ksplit = (a.total_ksteps + a.ksteps_per_slice - 1) / a.ksteps_per_slice;
    if (a.ksplit != d->ksplit)
      return std::to_string(a.total_ksteps) + " K steps are split over " + std::to_string(a.ksplit) + " slices, not " +
             std::to_string(d->ksplit);
  }
  return std::string();
}

xv_status xv_kernel_tdnn_gemm(const xv_gemm_desc* d) {
  if (!d) return Fail(XV_ERR_ARG, "xv_kernel_tdnn_gemm: null descriptor");
  return Guard([&] {
    xv::GemmArgs a;
    const std::string bad = GemmArgsFromDesc(d, &a);
    if (!bad.empty()) return Fail(XV_ERR_ARG, "xv_kernel_tdnn_gemm: " + bad);
    if (a.ksplit > 1) {
      void* ws = nullptr;
      hipError_t e = hipMalloc(&ws, (size_t)a.ksplit * d->rows * d->n_pad * 4);
      if (e != hipSuccess) return Fail(XV_ERR_DEVICE, std::string("hipMalloc(split-K workspace): ") + hipGetErrorString(e));
      a.splitk_ws = (float*)ws;
      e = xv::launch_tdnn_gemm(a, d->precision, d->epilogue, (hipStream_t)d->hip_stream);
      const hipError_t e2 = hipStreamSynchronize((hipStream_t)d->hip_stream);
      (void)hipFree(ws);
      if (e != hipSuccess || e2 != hipSuccess)
        return Fail(XV_ERR_DEVICE, std::string("tdnn_gemm split-K launch: ") + hipGetErrorString(e != hipSuccess ? e : e2));
      return XV_OK;
    }
    if (a.p8) {
      if (!xv::gemm_p8_applicable(a, d->precision) || (d->epilogue != xv::kEpiAct && d->epilogue != xv::kEpiStats))
        return Fail(XV_ERR_ARG, "xv_kernel_tdnn_gemm: p8 needs XV_PREC_FP16, XV_PREC_FP16MX or XV_PREC_FP16MX2, epilogue 0 or 2, rows and n_pad "
                                "multiples of 256, K groups of whole 64-column tiles (128-column blocks for XV_PREC_FP16MX, 256 for XV_PREC_FP16MX2)");
    } else
    if (d->precision == xv::kPrecFp16Mx2 && !xv::gemm_mx2_applicable(a))
      return Fail(XV_ERR_ARG, "xv_kernel_tdnn_gemm: XV_PREC_FP16MX2 needs what XV_PREC_FP16MX needs and the 4-bit planes of the "
                              "weights and of every source (whole 128-column steps)");
    if (!a.p8 && d->precision == xv::kPrecFp16Mx && !xv::gemm_mx_applicable(a))
      return Fail(XV_ERR_ARG, "xv_kernel_tdnn_gemm: XV_PREC_FP16MX needs the residual plane, a group-max table per source, "
                              "K groups of whole 128-column blocks and an even number of 128-row tiles");
    hipError_t e = xv::launch_tdnn_gemm(a, d->precision, d->epilogue, (hipStream_t)d->hip_stream);
    if (e != hipSuccess) return Fail(XV_ERR_DEVICE, std::string("tdnn_gemm launch: ") + hipGetErrorString(e));
    return XV_OK;
  });
}

static xv_status PlanGemmEntry(const char* who, const xv_gemm_desc* d, const xv::GemmPolicy& policy, xv_gemm_plan* out) {
  if (!d || !out) return Fail(XV_ERR_ARG, std::string(who) + ": null argument");
  return Guard([&] {
    memset(out, 0, sizeof *out);
    out->refused = 1;
    xv::GemmArgs a;
    if (!GemmArgsFromDesc(d, &a).empty()) return XV_OK;
    if (a.ksplit > 1) a.splitk_ws = (float*)out;   // never read: the plan only has to know that the launch entry brings a workspace
    const xv::GemmPlan p = xv::PlanGemm(a, d->precision, d->epilogue, policy);
    if (!p.ok) return XV_OK;
    const xv::GemmArgs& b = p.args;
    const bool persistent = p.kernel == xv::kGemmSk || p.kernel == xv::kGemmP8, v2 = p.kernel == xv::kGemmV2;
    out->refused = 0;
    xv::GemmKernelName(p, out->kernel, sizeof out->kernel);
    out->grid_x = p.grid_x;
    out->grid_y = p.grid_y;
    out->block = p.block;
    out->lds_bytes = p.lds;
    out->mf = p.mf;
    out->workspace_bytes = (int64_t)p.sk_ws_bytes;
    if (persistent) {
      out->lanes = b.sk_lanes;
      out->groups_per_xcd = p.grid_x / 8 / b.sk_lanes;
      out->sk_mtiles = b.sk_mtiles;
    }
    if (p.kernel == xv::kGemmP8) {
      out->p8_ktiles = b.p8_ktiles;
      out->p8_ktiles_lo = b.p8_ktiles_lo;
      out->p8_whole = b.p8_whole;
    }
    if (v2) out->stagger_units = b.stagger_units;
    if (p.kernel != xv::kGemmSplitK) {   // (tdnn_gemm_kernel walks K segment by segment: the groups are planned, not read)
      out->ngrp = b.ngrp;
      out->ngrp_lo = b.ngrp_lo;
      out->lo_ksteps = b.lo_ksteps;
      for (int i = 0; i < b.ngrp + b.ngrp_lo; ++i) {
        const xv::Grp& g = b.grp[i];
        out->grp[i] = {g.ld, g.ksteps, g.nshift, g.shift0, g.dstep, g.wcol0, g.wstride, g.ld4s};
      }
    }
    return XV_OK;
  });
}

xv_status xv_plan_gemm(const xv_gemm_desc* d, int32_t cus, xv_gemm_plan* out) {
  return PlanGemmEntry("xv_plan_gemm", d, cus > 0 ? xv::DefaultGemmPolicy(cus) : xv::CurrentGemmPolicy(), out);
}

xv_status xv_plan_gemm_policy(const xv_gemm_desc* d, int32_t cus, int32_t variant, int32_t sk_mf, int32_t sk_lanes, int32_t stagger_pct,
                              xv_gemm_plan* out) {
  return PlanGemmEntry("xv_plan_gemm_policy", d, xv::MakeGemmPolicy(cus, variant, sk_mf, sk_lanes, stagger_pct), out);
}

const char* xv_last_gemm_kernel(void) { return xv::last_gemm_kernel(); }

namespace {
// device memory of one test entry: freed when the entry returns
struct DevMem {
  void* p = nullptr;
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
  hipError_t Alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
};
}  // namespace

xv_status xv_kernel_first_layer(const xv_first_layer_desc* d) {
  if (!d) return Fail(XV_ERR_ARG, "xv_kernel_first_layer: null descriptor");
  return Guard([&] {
    const char* who = "xv_kernel_first_layer: ";
    if (!d->feats || !d->row_offsets || !d->dev_off || !d->w_hi || !d->w_lo || !d->bias || !d->out_hi || (d->bn && (!d->scale || !d->offset)))
      return Fail(XV_ERR_ARG, std::string(who) + "a required pointer is null");
    const int p = d->epi_prec;
    if (p != xv::kPrecBf16x3 && p != xv::kPrecFp16x3 && p != xv::kPrecFp16x2 && p != xv::kPrecFp16x3E)
      return Fail(XV_ERR_ARG, std::string(who) + "epi_prec must be XV_PREC_BF16X3, XV_PREC_FP16X3, XV_PREC_FP16X2 or XV_PREC_FP16X3E");
    if ((p == xv::kPrecBf16x3 || p == xv::kPrecFp16x3) && !d->out_lo) return Fail(XV_ERR_ARG, std::string(who) + "the split planes need out_lo");
    if (p == xv::kPrecFp16x3E && (!d->out_lo4 || !d->out_lo4_scale))
      return Fail(XV_ERR_ARG, std::string(who) + "XV_PREC_FP16X3E needs out_lo4 and out_lo4_scale");
    if (d->B < 1 || d->rows < xv::kFirstRows || d->rows % xv::kFirstRows || d->n_pad < xv::kBN || d->n_pad % xv::kBN ||
        d->ldo < d->n_pad || d->ldo % 64 || d->pad_left < 0 || d->pad_right < 0)
      return Fail(XV_ERR_ARG, std::string(who) + "bad geometry (rows: multiple of 64, n_pad: multiple of 128, ldo: multiple of 64, >= n_pad)");
    if (d->nrows < xv::kFirstRows || d->nrows % xv::kFirstRows || d->row0 < 0 || d->row0 % xv::kFirstRows || d->row0 + (long)d->nrows > d->rows)
      return Fail(XV_ERR_ARG, std::string(who) + "row0 and nrows must be multiples of 64 inside [0, rows]");
    if (d->dim < 1 || d->noff < 1 || d->noff > 8) return Fail(XV_ERR_ARG, std::string(who) + "dim >= 1 and 1 .. 8 offsets");
    int off[8];
    for (int j = 0; j < d->noff; ++j) {
      off[j] = d->off[j];
      if (off[j] < -15 || off[j] > 15) return Fail(XV_ERR_ARG, std::string(who) + "time offsets beyond +-15 frames");
    }
    if (!xv::FirstLayerApplicable(d->dim, d->noff, off))
      return Fail(XV_ERR_ARG, std::string(who) + "tdnn_first_kernel cannot run this shape (dim rounded up to 8 must be <= 24, noff x that <= 128, "
                                                 "and (64 + offset span) x that <= 2048)");
    if (d->seg_pad < d->dim || (long)(d->noff - 1) * d->seg_pad + d->dim > d->ldw)
      return Fail(XV_ERR_ARG, std::string(who) + "the weight planes do not hold noff segments of dim columns");
    // 16-row groups of the chunks
    const int ngrp = d->rows / xv::kRowAlign;
    std::vector<int32_t> grp_utt(ngrp, -1);
    long next_free = 0;
    if (d->row_offsets[0] < 0) return Fail(XV_ERR_ARG, std::string(who) + "negative row offset");
    for (int b = 0; b < d->B; ++b) {
      const long len = (long)d->row_offsets[b + 1] - d->row_offsets[b];
      const long span = (len + d->pad_left + d->pad_right + xv::kRowAlign - 1) / xv::kRowAlign * xv::kRowAlign;
      if (len < 1 || d->dev_off[b] % xv::kRowAlign || d->dev_off[b] < next_free || d->dev_off[b] + span > d->rows)
        return Fail(XV_ERR_ARG, std::string(who) + "chunk " + std::to_string(b) + ": empty, not on a 16-row boundary, overlapping or beyond rows");
      next_free = d->dev_off[b] + span;
      for (long g = d->dev_off[b] / xv::kRowAlign; g < next_free / xv::kRowAlign; ++g) grp_utt[g] = b;
    }
    std::vector<int32_t> grp_src((size_t)ngrp * 4);
    xv::FillFirstGroupSources(ngrp, grp_utt.data(), d->dev_off, d->row_offsets, d->pad_left, d->pad_right, grp_src.data());
    hipStream_t s = (hipStream_t)d->hip_stream;
    DevMem tab, wch, wcl;
    const size_t wc_bytes = (size_t)d->n_pad * xv::kFirstK * 2;
    hipError_t e = tab.Alloc(grp_src.size() * 4);
    if (e == hipSuccess) e = wch.Alloc(wc_bytes);
    if (e == hipSuccess) e = wcl.Alloc(wc_bytes);
    if (e == hipSuccess) e = hipMemcpy(tab.p, grp_src.data(), grp_src.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return Fail(XV_ERR_DEVICE, std::string("first_layer tables: ") + hipGetErrorString(e));
    xv::FirstArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.g.n_tiles = d->n_pad / xv::kBN;
    fa.g.m_tiles = d->rows / xv::kBM;
    fa.g.relu = d->relu;
    fa.g.bn = d->bn;
    fa.g.bias = d->bias;
    fa.g.scale = d->scale;
    fa.g.offset = d->offset;
    fa.g.out_hi = (uint16_t*)d->out_hi;
    fa.g.out_lo = (uint16_t*)d->out_lo;
    fa.g.ldo = d->ldo;
    fa.g.out_lo4 = (uint8_t*)d->out_lo4;
    fa.g.out_lo4s = (uint8_t*)d->out_lo4_scale;
    fa.g.gmax_out = (unsigned*)d->gmax_out;
    fa.g.out_range = d->out_range;
    fa.feats = d->feats;
    fa.feats_valid_idx = (long)d->row_offsets[0] * d->dim;
    fa.grp_src = (const int4*)tab.p;
    fa.rows = d->rows;
    fa.dim = d->dim;
    fa.row0 = d->row0;
    fa.nrows = d->nrows;
    fa.noff = d->noff;
    for (int j = 0; j < d->noff; ++j) fa.off[j] = off[j];
    fa.wc_hi = (const uint16_t*)wch.p;
    fa.wc_lo = (const uint16_t*)wcl.p;
    fa.max_wgs = d->max_wgs > 0 ? d->max_wgs : 0;
    e = xv::launch_compact_first((const uint16_t*)d->w_hi, d->ldw, d->seg_pad, d->n_pad, d->noff, d->dim, (uint16_t*)wch.p, s);
    if (e == hipSuccess) e = xv::launch_compact_first((const uint16_t*)d->w_lo, d->ldw, d->seg_pad, d->n_pad, d->noff, d->dim, (uint16_t*)wcl.p, s);
    if (e == hipSuccess) e = xv::launch_tdnn_first(fa, p, s);
    const hipError_t e2 = hipStreamSynchronize(s);   // the tables above are freed on return
    if (e != hipSuccess || e2 != hipSuccess)
      return Fail(XV_ERR_DEVICE, std::string("tdnn_first launch: ") + hipGetErrorString(e != hipSuccess ? e : e2));
    return XV_OK;
  });
}

xv_status xv_kernel_prep_input(const xv_prep_input_desc* d) {
  if (!d) return Fail(XV_ERR_ARG, "xv_kernel_prep_input: null descriptor");
  return Guard([&] {
    if (d->precision < xv::kPrecBf16x3 || d->precision > xv::kPrecFp16x3) return Fail(XV_ERR_ARG, "xv_kernel_prep_input: precision must be 0 .. 3");
    const bool split = xv::PrecXPlanes(d->precision) == 2;
    if (!d->feats || !d->src_off || !d->dev_off || !d->grp_utt || !d->out_hi || (split && !d->out_lo))
      return Fail(XV_ERR_ARG, "xv_kernel_prep_input: a required pointer is null");
    if (d->rows < xv::kBM || d->rows % xv::kBM || d->ld < xv::kBK || d->ld % xv::kBK || d->dim < 1 || d->dim > d->ld || d->pad_left < 0 ||
        d->pad_right < 0 || d->n_zero_words < 0 || (d->n_zero_words > 0 && !d->zero_words))
      return Fail(XV_ERR_ARG, "xv_kernel_prep_input: bad geometry (rows: multiple of 128, ld: multiple of 32, >= dim)");
    xv::PrepArgs a;
    memset(&a, 0, sizeof a);
    a.feats = d->feats;
    a.src_off = d->src_off;
    a.dev_off = d->dev_off;
    a.grp_utt = d->grp_utt;
    a.rows = d->rows;
    a.dim = d->dim;
    a.ld = d->ld;
    a.out_hi = (uint16_t*)d->out_hi;
    a.out_lo = (uint16_t*)d->out_lo;
    a.pad_left = d->pad_left;
    a.pad_right = d->pad_right;
    a.zero_words = (unsigned*)d->zero_words;
    a.n_zero_words = d->n_zero_words;
    const hipError_t e = xv::launch_prep_input(a, d->precision, (hipStream_t)d->hip_stream);
    if (e != hipSuccess) return Fail(XV_ERR_DEVICE, std::string("prep_input launch: ") + hipGetErrorString(e));
    return XV_OK;
  });
}

xv_status xv_kernel_pool_finalise(const xv_pool_finalise_desc* d) {
  if (!d) return Fail(XV_ERR_ARG, "xv_kernel_pool_finalise: null descriptor");
  return Guard([&] {
    if (d->precision < xv::kPrecBf16x3 || d->precision > xv::kPrecFp16x3) return Fail(XV_ERR_ARG, "xv_kernel_pool_finalise: precision must be 0 .. 3");
    const bool split = xv::PrecXPlanes(d->precision) == 2;
    if (!d->partial || !d->utt_grp0 || !d->utt_grp1 || !d->utt_count || !d->out_hi || (split && !d->out_lo))
      return Fail(XV_ERR_ARG, "xv_kernel_pool_finalise: a required pointer is null");
    if (d->B < 1 || d->dim < 1 || d->ldp < d->dim || d->ld < 2 * d->dim)
      return Fail(XV_ERR_ARG, "xv_kernel_pool_finalise: bad geometry (ldp >= dim, ld >= 2 dim)");
    xv::PoolArgs a;
    memset(&a, 0, sizeof a);
    a.partial = d->partial;
    a.ldp = d->ldp;
    a.utt_grp0 = d->utt_grp0;
    a.utt_grp1 = d->utt_grp1;
    a.utt_count = d->utt_count;
    a.B = d->B;
    a.dim = d->dim;
    a.var_floor = d->var_floor;
    a.out_hi = (uint16_t*)d->out_hi;
    a.out_lo = (uint16_t*)d->out_lo;
    a.ld = d->ld;
    const hipError_t e = xv::launch_pool_finalise(a, d->precision, (hipStream_t)d->hip_stream);
    if (e != hipSuccess) return Fail(XV_ERR_DEVICE, std::string("pool_finalise launch: ") + hipGetErrorString(e));
    return XV_OK;
  });
}

xv_status xv_kernel_frame_output(const xv_frame_output_desc* d) {
  if (!d) return Fail(XV_ERR_ARG, "xv_kernel_frame_output: null descriptor");
  return Guard([&] {
    if ((!d->src && !d->src16) || !d->out) return Fail(XV_ERR_ARG, "xv_kernel_frame_output: a required pointer is null");
    if (d->n_out < 1 || d->dim < 1 || d->ld < d->dim || d->out_ld < d->dim) return Fail(XV_ERR_ARG, "xv_kernel_frame_output: bad geometry");
    if (d->src16 && (!d->log_softmax || d->dim > 256 * 64))
      return Fail(XV_ERR_ARG, "xv_kernel_frame_output: fp16 logits are read by the log-softmax kernels only, rows of up to 16384 columns");
    xv::FrameOutArgs a;
    memset(&a, 0, sizeof a);
    a.src = d->src;
    a.src16 = (const uint16_t*)d->src16;
    a.ld = d->ld;
    a.out_row = d->out_row;
    a.n_out = d->n_out;
    a.dim = d->dim;
    a.log_softmax = d->log_softmax;
    a.out = d->out;
    a.out_ld = d->out_ld;
    const hipError_t e = xv::launch_frame_output(a, (hipStream_t)d->hip_stream);
    if (e != hipSuccess) return Fail(XV_ERR_DEVICE, std::string("frame_output launch: ") + hipGetErrorString(e));
    return XV_OK;
  });
}

xv_status xv_bucket_sort(int32_t device, const int32_t* keys, int64_t pairs, const int32_t* seg_off, int32_t num_segments,
                         int32_t num_keys, int32_t* bucket_start_out, int32_t* sorted_out) {
  if (!seg_off || !bucket_start_out || (pairs > 0 && (!keys || !sorted_out))) return Fail(XV_ERR_ARG, "xv_bucket_sort: null argument");
  return Guard([&] {
    for (int64_t i = 0; i < pairs; ++i)   // the input comes from outside: the kernels index the histogram with the keys
      if (keys[i] < 0 || keys[i] >= num_keys)
        return Fail(XV_ERR_ARG, "xv_bucket_sort: key " + std::to_string(keys[i]) + " is outside [0, " + std::to_string(num_keys) + ")");
    xv::UseDevice(device, "the bucket sort needs");
    xv::DevBuf d_keys;
    if (pairs > 0) d_keys.Upload(keys, (size_t)pairs * 4, "copy the keys");
    xv::BucketSorter sort;
    const hipError_t e = sort.Run(d_keys.as<int32_t>(), pairs, seg_off, num_segments, num_keys, nullptr);
    if (e == hipErrorInvalidValue) return Fail(XV_ERR_ARG, "xv_bucket_sort: sizes or a segment table that the sort does not take");
    if (e != hipSuccess) return Fail(XV_ERR_DEVICE, std::string("bucket_sort launch: ") + hipGetErrorString(e));
    xv::Check(hipDeviceSynchronize(), "bucket_sort");
    sort.start.Download(bucket_start_out, (size_t)num_segments * (num_keys + 1) * 4, "copy the bucket table");
    if (pairs > 0) sort.sorted.Download(sorted_out, (size_t)pairs * 4, "copy the sorted pairs");
    return XV_OK;
  });
}

static xv_status PackMxResidualImpl(bool walk64, const float* w, const uint16_t* w_hi_f16, int32_t n_pad, int32_t nseg,
                                    const int32_t* seg_src, const int32_t* seg_shift, const int32_t* seg_klen, uint8_t* w4,
                                    uint8_t* w4_scale) {
  if (!w || !w_hi_f16 || !seg_src || !seg_shift || !seg_klen || !w4 || !w4_scale || nseg < 1 || nseg > xv::kMaxSeg || n_pad < 1)
    return Fail(XV_ERR_ARG, "xv_pack_mx_residual: bad argument");
  return Guard([&] {
    long key[xv::kMaxSeg];
    int shift[xv::kMaxSeg], ksteps[xv::kMaxSeg], k_pad = 0;
    for (int j = 0; j < nseg; ++j) {
      if (seg_klen[j] % xv::kBK) return Fail(XV_ERR_ARG, "xv_pack_mx_residual: k_len must be a multiple of 32");
      key[j] = seg_src[j];
      shift[j] = seg_shift[j];
      ksteps[j] = seg_klen[j] / xv::kBK;
      k_pad += seg_klen[j];
    }
    xv::WalkGroup wg[xv::kMaxSeg];
    const int ng = xv::PlanWalkGroups(nseg, key, shift, ksteps, wg);
    std::vector<int> step_wcol(k_pad / xv::kBK);
    bool ok = false;
    if (walk64) xv::PlanWalkSteps64(ng, wg, step_wcol.data(), (int)step_wcol.size(), &ok);
    else xv::PlanWalkSteps(ng, wg, step_wcol.data(), (int)step_wcol.size(), &ok);
    if (!ok) return Fail(XV_ERR_ARG, "xv_pack_mx_residual: a K group is not a multiple of four steps");
    const int ldw4 = k_pad / xv::kBK / 4 * 64;
    std::vector<float> res(k_pad);
    for (int n = 0; n < n_pad; ++n) {
      for (int k = 0; k < k_pad; ++k) res[k] = w[(size_t)n * k_pad + k] - xv::host_f16_to_f32(w_hi_f16[(size_t)n * k_pad + k]);
      xv::PackMxRow(res.data(), k_pad, step_wcol.data(), w4 + (size_t)n * ldw4, w4_scale + (size_t)n * (k_pad / xv::kBK));
    }
    return XV_OK;
  });
}

xv_status xv_pack_mx_residual(const float* w, const uint16_t* w_hi_f16, int32_t n_pad, int32_t nseg, const int32_t* seg_src,
                              const int32_t* seg_shift, const int32_t* seg_klen, uint8_t* w4, uint8_t* w4_scale) {
  return PackMxResidualImpl(false, w, w_hi_f16, n_pad, nseg, seg_src, seg_shift, seg_klen, w4, w4_scale);
}

xv_status xv_pack_mx_residual64(const float* w, const uint16_t* w_hi_f16, int32_t n_pad, int32_t nseg, const int32_t* seg_src,
                                const int32_t* seg_shift, const int32_t* seg_klen, uint8_t* w4, uint8_t* w4_scale) {
  return PackMxResidualImpl(true, w, w_hi_f16, n_pad, nseg, seg_src, seg_shift, seg_klen, w4, w4_scale);
}

static xv_status PackMxWeightsImpl(bool walk64, const float* w, int32_t n_pad, int32_t nseg, const int32_t* seg_src,
                                   const int32_t* seg_shift, const int32_t* seg_klen, uint8_t* w4b, uint8_t* w4b_scale) {
  if (!w || !seg_src || !seg_shift || !seg_klen || !w4b || !w4b_scale || nseg < 1 || nseg > xv::kMaxSeg || n_pad < 1)
    return Fail(XV_ERR_ARG, "xv_pack_mx_weights: bad argument");
  return Guard([&] {
    long key[xv::kMaxSeg];
    int shift[xv::kMaxSeg], ksteps[xv::kMaxSeg], k_pad = 0;
    for (int j = 0; j < nseg; ++j) {
      if (seg_klen[j] % (walk64 ? 256 : 128)) return Fail(XV_ERR_ARG, "xv_pack_mx_weights: k_len must be a multiple of 128 (256 for the p8 order)");
      key[j] = seg_src[j];
      shift[j] = seg_shift[j];
      ksteps[j] = seg_klen[j] / xv::kBK;
      k_pad += seg_klen[j];
    }
    xv::WalkGroup wg[xv::kMaxSeg];
    const int ng = xv::PlanWalkGroups(nseg, key, shift, ksteps, wg);
    std::vector<int> lo_wcol(k_pad / 128);
    const int n_lo = walk64 ? xv::PlanWalkLoSteps64(ng, wg, lo_wcol.data(), (int)lo_wcol.size())
                            : xv::PlanWalkLoSteps(ng, wg, lo_wcol.data(), (int)lo_wcol.size());
    if (n_lo != (int)lo_wcol.size()) return Fail(XV_ERR_ARG, "xv_pack_mx_weights: inconsistent walk");
    const size_t pitch = walk64 ? (size_t)k_pad * 2 : (size_t)n_lo * 64;   // p8: rows of the fp16 plane's pitch
    if (walk64) memset(w4b, 0, pitch * n_pad);
    for (int n = 0; n < n_pad; ++n)
      xv::PackMxWeightsRow(w + (size_t)n * k_pad, lo_wcol.data(), n_lo, w4b + (size_t)n * pitch, w4b_scale + (size_t)n * n_lo * 4);
    return XV_OK;
  });
}

xv_status xv_pack_mx_weights(const float* w, int32_t n_pad, int32_t nseg, const int32_t* seg_src, const int32_t* seg_shift,
                             const int32_t* seg_klen, uint8_t* w4b, uint8_t* w4b_scale) {
  return PackMxWeightsImpl(false, w, n_pad, nseg, seg_src, seg_shift, seg_klen, w4b, w4b_scale);
}

xv_status xv_pack_mx_weights64(const float* w, int32_t n_pad, int32_t nseg, const int32_t* seg_src, const int32_t* seg_shift,
                               const int32_t* seg_klen, uint8_t* w4b, uint8_t* w4b_scale) {
  return PackMxWeightsImpl(true, w, n_pad, nseg, seg_src, seg_shift, seg_klen, w4b, w4b_scale);
}

xv_status xv_tile_mx_scales(const uint8_t* natural, int32_t n_pad, int32_t k_len, int32_t epilogue, uint8_t* tiled) {
  if (!natural || !tiled || n_pad < 1 || n_pad % xv::kBN || k_len < 128 || k_len % 128)
    return Fail(XV_ERR_ARG, "xv_tile_mx_scales: bad argument");
  return Guard([&] {
    xv::TileMxScales(natural, n_pad, k_len / xv::kBK, epilogue != xv::kEpiStats, tiled);
    return XV_OK;
  });
}

}  // extern "C"
