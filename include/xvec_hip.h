/* xvec_hip.h - C ABI of the MI355X-native x-vector / c-vector embedding extractor.
 *
 * The reference (mycrazycracy/speaker-embedding-with-phonetic-information) has no plugin, operator or
 * FFI interface for this path: its boundary is the command line of Kaldi's `nnet3-xvector-compute`
 * (call sites egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:86-87,92-93) plus Kaldi's file
 * formats.  The drop-in for that boundary is the `nnet3-xvector-compute` executable built from
 * csrc/nnet3_xvector_compute_main.cc; this header is the C ABI *underneath* it, i.e.
 * what a maintainer who wants to call the extractor from a host language binds.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types; the caller owns every host buffer;
 * the library owns device memory; no exception crosses the boundary (every entry returns xv_status and
 * the message is available from xv_last_error(), thread-local); an xv_ctx may be used by one thread at
 * a time, different xv_ctx objects are independent.  There is NO CPU compute path behind this ABI:
 * creating a context without a gfx950 device fails with XV_ERR_DEVICE.
 */
#ifndef XVEC_HIP_H_
#define XVEC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  XV_OK = 0,
  XV_ERR_IO = 1,       /* unreadable rxfilename / malformed Kaldi object */
  XV_ERR_MODEL = 2,    /* graph outside the supported TDNN grammar */
  XV_ERR_DEVICE = 3,   /* no gfx950 device, HIP failure */
  XV_ERR_ARG = 4,      /* invalid argument (e.g. a chunk shorter than the network context) */
  XV_ERR_INTERNAL = 5
} xv_status;

typedef enum {
  XV_PREC_DEFAULT = -1, /* the policy of the command-line tools, and what every entry point of this library defaults to:
                          the context is PACKED as XV_PREC_FP16MX2 for a pooled (x-vector) output whose layers can all
                          run it, XV_PREC_FP16X3 otherwise (a layer the 4-bit walk cannot cover, frame-level outputs);
                          xv_ctx_info reports that mode.  On its own this meets the parity bar on every model tried,
                          heavy-tailed ones included.  A context packed this way can be
                          CALIBRATED (xv_ctx_calibrate / xv_calibrate_table; the command-line tools and dist_extract.py
                          do it by default, xv_forward_batch users only when they call it): it then runs the lighter,
                          model-dependent XV_PREC_FP16MX where - and only where - that was measured within the
                          tolerance on a sample of the job's own data; xv_ctx_fast_mode reports what it runs */
  XV_PREC_BF16X3 = 0,  /* split-bf16 MFMA (3 products, fp32 accumulate): fp32-grade, the first version's parity mode */
  XV_PREC_BF16 = 1,    /* single-pass bf16 MFMA */
  XV_PREC_FP16 = 2,    /* single-pass fp16 MFMA */
  XV_PREC_FP16X3 = 3,  /* split-fp16 MFMA (3 products of 11+11-bit operands, fp32 accumulate) */
  XV_PREC_FP16X2 = 4,  /* fp16 activations x split-fp16 weights (2 products): removes the weight rounding error, which
                          is coherent over the frames of a chunk; the activation rounding error averages out in the
                          statistics pooling.  Layers after the pooling run XV_PREC_FP16X3.  Not for frame-level
                          outputs (they run XV_PREC_FP16X3) */
  XV_PREC_AUTO = 5,    /* XV_PREC_FP16MX for chunks that pool >= 300 frames (XVEC_FAST_MIN_POOLED), XV_PREC_FP16X3 for
                          shorter ones; the choice depends on the chunk's own length only */
  XV_PREC_FP16MX = 6,  /* XV_PREC_FP16X2 with the second product (activations x weight residual) done on block-scaled
                          4-bit operands at four times the fp16 MFMA rate (v_mfma_scale_f32_16x16x128_f8f6f4): 1.25
                          passes per product.  The residual term is 2^-11 of the product and only has to be good to
                          ~4 bits.  Layers whose K length is not a multiple of 128 run XV_PREC_FP16X2 */
  XV_PREC_FP16MX2 = 7, /* XV_PREC_FP16MX plus a block-scaled 4-bit product for what the fp16 rounding of the ACTIVATIONS
                          dropped (the producing layer writes that residual as a 4-bit plane): 1.5 passes per product,
                          error independent of how well the pooling averages the activation rounding.  Layers whose K
                          length is not a multiple of 128 run XV_PREC_FP16X3E */
  XV_PREC_FP16X3E = 8, /* kernel mode of XV_PREC_FP16MX2 passes: XV_PREC_FP16X3 whose planes epilogue writes the fp16
                          plane + its 4-bit residual instead of two fp16 planes */
  XV_PREC_FP16MXE = 9  /* kernel mode of XV_PREC_FP16MX2 passes: XV_PREC_FP16MX whose planes epilogue writes the fp16 plane +
                          its 4-bit residual (a "lite" layer, xv_calibration.lite_mask, in front of a 1.5-pass consumer) */
} xv_precision;

typedef struct xv_model xv_model; /* host side: parsed nnet3 model lowered to a TDNN program */
typedef struct xv_ctx xv_ctx;     /* device side: weights resident on one GPU + workspaces + stream */

typedef struct {
  int32_t input_dim;         /* feature dimension (23 in egs/sre, conf/mfcc.conf:5) */
  int32_t output_dim;        /* embedding dimension (512) */
  int32_t left_context;      /* frames not computable at the left edge of a chunk (7 / 13) */
  int32_t right_context;     /* ... at the right edge (7) */
  int32_t min_frames;        /* smallest chunk with >= 1 pooled frame (15 / 21) */
  int32_t num_layers;        /* affine layers in the dependency cone of the output */
  int32_t output_is_segment; /* 1: one vector per chunk (x-vector); 0: one row per frame */
  int32_t reserved;
} xv_model_info_t;

/* Message of the last failure on the calling thread ("" if none). */
const char* xv_last_error(void);
const char* xv_version(void);

/* ---- model (replaces ReadKaldiObject + SetBatchnormTestMode + CollapseModel + Compile) -------------
 * raw/n: the bytes of an nnet3 "raw" model, binary or text (what `$srcdir/final.raw` holds,
 *        extract_xvectors_new.sh:53).
 * nnet_config: optional text applied like `nnet3-copy --nnet-config=<file>` (extract_xvectors_new.sh:58-59
 *        writes "output-node name=output input=tdnn6.affine" into extract.config); may be NULL.
 * output_node: name of the output-node to compute; NULL means "output". */
xv_status xv_model_load(const void* raw, size_t n, const char* nnet_config, const char* output_node,
                        xv_model** out);
/* Same, reading a Kaldi rxfilename: "file", "file:offset", "-", or "command |" (the form every recipe
 * call uses: "nnet3-copy --nnet-config=... final.raw - |"). */
xv_status xv_model_load_rxfilename(const char* rxfilename, const char* nnet_config, const char* output_node,
                                   xv_model** out);
void xv_model_free(xv_model* m);
xv_status xv_model_info(const xv_model* m, xv_model_info_t* info);
/* Algorithmic multiply-accumulates of one chunk of `frames` frames (unpadded dims, only the frames
 * nnet3 would compute). */
double xv_model_macs(const xv_model* m, int32_t frames);
/* Human-readable layer table; returns the number of bytes needed (including the NUL). */
size_t xv_model_describe(const xv_model* m, char* buf, size_t n);
/* Packed, padded, precision-split weight image: what one rank broadcasts to the others over RCCL
 * (SURVEY.md §8(e)).  Call with blob == NULL to get the size. */
xv_status xv_model_pack(const xv_model* m, int precision, void* blob, size_t* nbytes);

/* ---- device context ---------------------------------------------------------------------------- */
xv_status xv_ctx_create(const xv_model* m, int device, int precision, xv_ctx** out);
xv_status xv_ctx_create_from_blob(const void* blob, size_t nbytes, int device, xv_ctx** out);
/* Same, the packed image being DEVICE memory on `device` (what a rank holds after the RCCL broadcast of the weights,
 * SURVEY.md section 8(e)): the weights go device to device, only the header and layer table are read back. */
xv_status xv_ctx_create_from_device_blob(const void* blob_dev, size_t nbytes, int device, xv_ctx** out);
void xv_ctx_free(xv_ctx* c);
xv_status xv_ctx_info(const xv_ctx* c, xv_model_info_t* info, int32_t* precision, int32_t* device);

/* One forward pass over a batch of B chunks (replaces RunNnetComputation for B chunks at once).
 * feats: packed rows [row_offsets[B]][input_dim] fp32; chunk b = rows row_offsets[b] .. row_offsets[b+1]-1;
 * out: [B][output_dim] fp32.  Every chunk must have >= min_frames rows (XV_ERR_ARG otherwise; nnet3
 * would refuse to compile the same request).  Host-buffer flavour: blocking.
 * Frame-level models (xv_model_info_t.output_is_segment == 0: the output node does not follow the statistics pooling,
 * e.g. senone log-posteriors `output.log-softmax` or bottleneck features `tdnn5.batchnorm`; what the reference gets
 * from `nnet3-compute`, sid/nnet3_cvector/cvector/extract_log_post.sh:77-84, sid/nnet3_cvector/am/extract_bn.sh:68):
 * the output has ONE ROW PER INPUT FRAME - chunk b occupies rows row_offsets[b]..row_offsets[b+1]-1 of out, exactly
 * like its features - the chunk being extended by replicating its first / last frame over the network's left / right
 * context (nnet3-compute's edge behaviour); any chunk length >= 1 is accepted. */
xv_status xv_forward_batch(xv_ctx* c, const float* feats, const int32_t* row_offsets, int32_t B, float* out);
/* Device-buffer flavour: feats/out are device pointers on the context's GPU, row_offsets is a HOST array;
 * asynchronous on hip_stream (a hipStream_t, NULL = the context's own stream). out rows are out_ld apart. */
xv_status xv_forward_batch_device(xv_ctx* c, const float* feats_dev, const int32_t* row_offsets, int32_t B,
                                  float* out_dev, int32_t out_ld, void* hip_stream);
/* Waits for everything the context launched, on its own streams and on callers' streams, and reports what only shows
 * once the kernels ran: XV_ERR_DEVICE if a persistent GEMM launch gave up waiting for another workgroup's partial tile
 * (results of that launch are invalid; xv_last_error() says how to select the per-tile kernels).  A caller of
 * xv_forward_batch_device on its own stream calls this before trusting the results. */
xv_status xv_ctx_synchronize(xv_ctx* c);
/* Per-kernel timing with HIP events recorded on the stream the kernels are launched on (used by bench.py for
 * the roofline figure).  xv_ctx_profile_report synchronises, writes "label<TAB>launches<TAB>total_ms" lines for
 * everything recorded since the previous report into buf (NUL terminated), resets the record, and returns
 * the number of bytes needed; call it often enough - every recorded forward keeps a handful of events alive. */
/* ---- calibrated arithmetic -----------------------------------------------------------------------------------------
 * A context packed as XV_PREC_FP16MX2 (what XV_PREC_DEFAULT resolves to for a pooled output) can also run the lighter
 * XV_PREC_FP16MX arithmetic (1.25 instead of 1.5 MFMA passes, +30 % throughput) and the three-pass XV_PREC_FP16X3 on the
 * same packed weights.  XV_PREC_FP16MX meets the parity bar on some models only, so it is never
 * assumed: xv_ctx_calibrate runs the caller's own chunks in all three, compares the embeddings of the two fast modes with
 * the three-pass ones (worst max|d| / max|ref|; XV_PREC_FP16MX over the chunks that pool >= 300 frames - the others run
 * three-pass in that mode -, XV_PREC_FP16MX2 over every chunk it runs fast, from 160 pooled frames) and switches the context to
 * XV_PREC_FP16MX only when at least 16 such chunks were compared, its worst chunk stays within tol (the tools use 7.5e-5: three
 * quarters of the 1e-4 bar) AND the tail its errors project (mean + 6 standard deviations over those chunks, xv_calibration.tail)
 * stays within tol x 1.10 - over 32 768 chunks the worst one was measured 4.6-5.9 standard deviations above the mean
 * (profiles/r05_tail_error.md) -, else leaves XV_PREC_FP16MX2
 * (or drops to XV_PREC_FP16X3 should even that exceed 1e-4 on a sampled chunk, or project a tail beyond tol x 1.20).  Contexts that cannot switch report their precision with
 * checked = 0.  (No reference counterpart: Kaldi computes in fp32 throughout.)  A measured choice depends on the sample it was
 * measured on, so the command-line tools never make one per job by default - `--precision=default` is plain XV_PREC_FP16MX2, a
 * function of the model alone - and use a measured choice only when it is SHARED between the jobs of a recipe through a
 * calibration file (xv_ctx_share_calibration below; `--calibration=<file>` / $XVEC_CALIBRATION).  xv_ctx_set_fast_mode applies a choice made elsewhere
 * (the other ranks of a multi-GPU job); xv_calibrate_table calibrates on max_utts utterances of a table: spread evenly
 * over the whole list where its objects can be addressed (archive file, script file - the reference's lists are sorted
 * by speaker, utils/data/split_data.sh:18-21, so the head of a list is one or two speakers), the head of a stream. */
typedef struct {
  int32_t chosen;   /* xv_precision the context now runs its fast chunks in */
  int32_t checked;  /* chunks compared */
  float err_mx;     /* XV_PREC_FP16MX against XV_PREC_FP16X3 */
  float err_mx2;    /* XV_PREC_FP16MX2 against XV_PREC_FP16X3 */
  int32_t checked_mx;  /* of them, chunks XV_PREC_FP16MX would run fast (what err_mx was measured on; fewer than 16: not chosen) */
  float err_lite;      /* chosen == XV_PREC_FP16MX2 with lite_mask != 0: error of that mixture over ALL checked_mx chunks */
  uint64_t lite_mask;  /* chosen == XV_PREC_FP16MX2: the layers (bit = index in xv_model_describe's table) that compute in 1.25 passes
                          inside the 1.5-pass context - where XV_PREC_FP16MX as a whole misses tol, the calibration keeps the
                          second walk (the correction of the activations' fp16 rounding) only on the layers that need it and
                          takes it off the most expensive ones the tolerance allows; 0: none.  The mixture is SELECTED on the
                          chunks at even positions of the sample and CONFIRMED on those at odd positions, which took no part
                          in the selection: layers are dropped again, last added first, until the held-out half is within tol */
  float err_holdout;        /* error of the adopted mixture over the held-out half (what confirmed it) */
  int32_t checked_holdout;  /* chunks of the held-out half XV_PREC_FP16MX would run fast */
  int32_t lite_dropped;     /* layers the selection half admitted and the held-out half threw out again */
  float tail;               /* projected tail of the per-chunk error of what was adopted: mean + 6 standard deviations over the
                               chunks that confirmed it (the whole sample; a mixture: its held-out half), never below their worst.
                               A configuration is adopted only while this is within tol x 1.10 (7.5e-5 -> 8.25e-5: the projection has
                               been measured up to 10 % below the worst of 32 768 chunks, profiles/r05_tail_error.md) */
} xv_calibration;
xv_status xv_ctx_calibrate(xv_ctx* c, const float* feats, const int32_t* row_offsets, int32_t B, float tol, xv_calibration* out);
xv_status xv_ctx_set_fast_mode(xv_ctx* c, int32_t precision);   /* also clears the lite layers */
xv_status xv_ctx_fast_mode(const xv_ctx* c, int32_t* precision);
/* The lite layers of a context running XV_PREC_FP16MX2 (xv_calibration.lite_mask): set applies a choice made elsewhere
 * (bits of layers that cannot run the 1.25-pass arithmetic are dropped; XV_ERR_ARG in any other fast mode), get reports it.
 * The mask has 64 bits: a layer with index >= 64 in xv_model_describe's table is never lite (the reference's deepest graph on
 * this path has 13 layers). */
xv_status xv_ctx_set_lite_layers(xv_ctx* c, uint64_t mask);
xv_status xv_ctx_lite_layers(const xv_ctx* c, uint64_t* mask);
xv_status xv_calibrate_table(xv_ctx* c, const char* feature_rspecifier, int32_t chunk_size, int32_t min_chunk_size,
                             int32_t pad_input, int32_t max_utts, float tol, xv_calibration* out);
/* xv_extract_table calibrates on a sample of its own table first (as xv_calibrate_table) when this is enabled (default: off) */
xv_status xv_ctx_set_calibration(xv_ctx* c, int32_t enable, float tol);
/* ---- the shared choice of a recipe (csrc/calib_file.h) -------------------------------------------------------------------
 * The reference splits a list over `nj` independent processes and concatenates their outputs
 * (egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:72,91-99); an utterance gets the same vector in whatever shard it lands.
 * For that to hold here, a MEASURED choice of arithmetic must be one choice for all jobs: a small text file beside the model
 * ("xvec-calibration 1", the fingerprint of the packed model image, the arithmetic, the mask of lite layers, provenance).
 * xv_ctx_model_fingerprint: the fingerprint of the context's packed image (part of the image header, so a context built from a
 * broadcast image knows it too).  xv_ctx_share_calibration: the file exists -> its choice is applied to the context
 * (*outcome = 0; XV_ERR_IO when it names another model image or cannot be parsed); it does not -> the context's CURRENT choice
 * (after xv_ctx_calibrate / xv_calibrate_table, or the packed default) is published atomically (temporary file + link(2): the
 * first of several concurrent publishers wins) and what the file then holds is applied: *outcome = 1 when this context's
 * choice was published, 2 when another job's was adopted.  note: one line of provenance written into the file (may be NULL).
 * xv_ctx_set_calibration_file: xv_extract_table does the same before its first batch (file present: applied, nothing measured;
 * absent: measured on the job's own sample, published, adopted).  NULL / "" turns it off.
 * xv_calibration_file_read / _publish: the file itself, without a context (no device call): read reports *found = 0 for a
 * missing file; publish writes (model, precision, lite_mask) unless the file exists and reports what the file then holds. */
xv_status xv_calibration_file_read(const char* path, int32_t* found, uint64_t* model, int32_t* precision, uint64_t* lite_mask);
xv_status xv_calibration_file_publish(const char* path, uint64_t model, int32_t precision, uint64_t lite_mask, float tol,
                                      const char* note, int32_t* published, uint64_t* adopted_model, int32_t* adopted_precision,
                                      uint64_t* adopted_lite_mask);
xv_status xv_ctx_model_fingerprint(const xv_ctx* c, uint64_t* fingerprint);
xv_status xv_ctx_share_calibration(xv_ctx* c, const char* path, float tol, const char* note, int32_t* outcome);
xv_status xv_ctx_set_calibration_file(xv_ctx* c, const char* path);

xv_status xv_ctx_set_profiling(xv_ctx* c, int32_t enable);
size_t xv_ctx_profile_report(xv_ctx* c, char* buf, size_t n);

/* The per-utterance loop of nnet3-xvector-compute (chunking + length-weighted average):
 * utterance u = rows row_offsets[u] .. row_offsets[u+1]-1 of feats (host).  chunk_size <= 0 means the whole
 * utterance; pad_input != 0 replicates edge frames of chunks shorter than min_chunk_size, pad_input == 0
 * skips them.  ok[u] = 1 if an embedding was written to out[u][:], 0 if the utterance counts as failed
 * (zero frames, too short).  Blocking. */
xv_status xv_extract_utterances(xv_ctx* c, const float* feats, const int32_t* row_offsets, int32_t n_utts,
                                int32_t chunk_size, int32_t min_chunk_size, int32_t pad_input, float* out,
                                int32_t* ok);

/* The whole job of one nnet3-xvector-compute process on an existing context: read a Kaldi feature table
 * (rspecifier, e.g. "scp:feats.scp" or "ark:apply-cmvn-sliding ... |"), extract, write a vector table
 * (wspecifier, e.g. "ark,scp:xvector.1.ark,xvector.1.scp").  Per-utterance problems are warnings on stderr and
 * are counted in *num_failed; the call fails only for fatal I/O or device errors.  batch_frames <= 0: default.
 * This is what a multi-GPU launcher calls per rank after the weights were broadcast. */
xv_status xv_extract_table(xv_ctx* c, const char* feature_rspecifier, const char* vector_wspecifier, int32_t chunk_size,
                           int32_t min_chunk_size, int32_t pad_input, int32_t batch_frames, int64_t* num_done,
                           int64_t* num_failed);

/* Feature front-end on the device (the two pipe stages of extract_xvectors_new.sh:79): sliding-window cepstral mean
 * subtraction (`apply-cmvn-sliding --norm-vars=false --center=<center> --cmn-window=<cmn_window>`; cmn_window <= 0: none)
 * over each whole utterance, then `select-voiced-frames` with vad[r] != 0 (vad: one float per raw row, NULL = keep
 * all).  raw: packed rows, utterance u = rows raw_off[u]..raw_off[u+1]-1; out receives the kept rows (capacity >= the
 * number of raw rows), out_off[n_utts+1] their offsets.  Host buffers, blocking. */
/* The feature pipeline every extraction script of the reference builds - "ark:apply-cmvn-sliding --norm-vars=false
 * --center=true --cmn-window=300 scp:feats.scp ark:- | select-voiced-frames ark:- scp,s,cs:vad.scp ark:- |"
 * (egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:79 and its siblings) - recognised as text (csrc/fuse_pipe.h): *found = 1
 * and the inner feature table, the VAD table ("" when there is no selection stage) and the sliding-CMN parameters when the string
 * is exactly that pipeline with options the device front-end implements; *found = 0 for anything else.  nnet3-xvector-compute
 * uses it to run the two stages on the device instead of as two CPU tools and two pipes. */
xv_status xv_recognize_feature_pipeline(const char* rspecifier, int32_t* found, char* feats, size_t feats_cap, char* vad, size_t vad_cap,
                                        int32_t* cmn_window, int32_t* min_cmn_window, int32_t* center);
xv_status xv_frontend_cmvn_select(xv_ctx* c, const float* raw, const int32_t* raw_off, int32_t n_utts, const float* vad,
                                  int32_t cmn_window, int32_t center, float* out, int32_t* out_off);

/* Host-only: the chunk list nnet3-xvector-compute would build for one utterance of num_rows frames
 * (SURVEY.md App. B.5).  Arrays of capacity `cap` receive per chunk: first source row, frames taken (= averaging
 * weight), copies of the first / last frame added by --pad-input.  *n_chunks = number of chunks; returns XV_ERR_ARG
 * with the reason in xv_last_error() when the utterance counts as failed (0 frames, too short). */
xv_status xv_plan_chunks(int32_t num_rows, int32_t chunk_size, int32_t min_chunk_size, int32_t pad_input,
                         int32_t min_net_frames, int32_t cap, int32_t* start, int32_t* len, int32_t* left_pad,
                         int32_t* right_pad, int32_t* n_chunks);

/* ---- multi-GPU: weights read once, broadcast over RCCL/xGMI --------------------------
 * Single-process form: creates one context per device in devices[0..n) from the model, reading/packing once
 * on the host, uploading to devices[0] and broadcasting device-to-device with one ncclBroadcast (n == 1 included:
 * a one-rank communicator; every context is built from the bytes its device received, without a host round trip). */
xv_status xv_ctx_create_broadcast(const xv_model* m, const int* devices, int n, int precision, xv_ctx** out);

/* ---- speaker-level back-end ----------------------------------------------
 * What the reference does to the vectors right after extraction, as device kernels behind host buffers
 * (no Kaldi FFI exists for these either; they replace the processes of egs/sre/v2/run_sre10.sh:238-241 and
 * egs/sre/v2/sid/nnet3/xvector/extract_xvectors_new.sh:106-107):
 *   xv_backend_apply   ivector-subtract-global-mean (mean != NULL) -> transform-vec (transform != NULL; t_cols == dim
 *                      linear, dim + 1 affine, anything else XV_ERR_ARG "Dimension mismatch") ->
 *                      ivector-normalize-length (normalize != 0; scaleup as Kaldi's --scaleup).
 *                      out[n][out_dim], out_dim = transform ? t_rows : dim; ratio[n] (optional) = |y|/sqrt(out_dim)
 *                      (|y| without scaleup) before normalisation; a zero vector is left unchanged (ratio 0).
 *   xv_segment_mean    ivector-mean: out[s] = mean of rows idx[seg_off[s] .. seg_off[s+1]) of x, added in list order,
 *                      fp32 accumulator (speaker means) or fp64 (acc64 != 0, the global mean); empty segment -> zeros.
 * Both fail with XV_ERR_DEVICE when no gfx950 device is usable. */
xv_status xv_backend_apply(int device, const float* x, int32_t n, int32_t dim, const float* mean, const float* transform,
                           int32_t t_rows, int32_t t_cols, int32_t normalize, int32_t scaleup, float* out, float* ratio);
xv_status xv_segment_mean(int device, const float* x, int32_t n, int32_t dim, const int32_t* seg_off, const int32_t* idx,
                          int32_t n_seg, int32_t acc64, float* out);

/* ---- PLDA back-end (stage 7 of egs/sre/v2/run_sre10.sh: ivector-compute-lda, ivector-compute-plda, ivector-plda-scoring;
 * stage 2 of v2/run_sre16.sh: ivector-adapt-plda)
 * Device kernels behind host buffers, fp64 arithmetic on fp32 vectors, deterministic (fixed reduction orders, no float
 * atomics).  device_ms (optional, may be NULL) receives the kernel time between two events around the launches.
 *   xv_scatter_stats   segment s = rows idx[seg_off[s] .. seg_off[s+1]) of x [n][dim] (seg_off[0] == 0, offsets do not
 *                      decrease, every index in [0, n)): s_tot[dim][dim] = sum of x_i x_i^T over every listed row,
 *                      sums[n_seg][dim] = per-segment sums (list order), s_bet[dim][dim] = sum_s sums_s sums_s^T / n_s.
 *                      Any output may be NULL.  dim up to 3000 and beyond (the workspace is dim^2 doubles per row chunk).
 *   xv_plda_transform  Kaldi's Plda::TransformIvector: y = offset + transform x (fp64, transform [dim][dim] row-major),
 *                      scale = sqrt(dim / sum_d y_d^2 / (psi_d + 1/num_i)) (simple != 0: sqrt(dim) / |y|), y *= scale
 *                      when normalize != 0; y[n][dim] stored as fp32, scale[n] (optional) as fp64.  dim <= 512.
 *   xv_plda_score      Kaldi's Plda::LogLikelihoodRatio of trial i = (enrolment row trials[2i] of u [n_u][dim] with
 *                      num_u examples, test row trials[2i+1] of v [n_v][dim]) into scores[i] (fp64).  An index out of
 *                      range is XV_ERR_ARG.  dim <= 512.
 *   xv_lda_estimate    host only (no GPU needed): ivector-compute-lda from the scatter statistics of n mean-subtracted
 *                      vectors; out[lda_dim][dim + 1] = [L | -L mean]; n_floored (optional) = eigenvalues floored in the
 *                      normalising transform.
 *   xv_plda_estimate   host only: ivector-compute-plda's EM (num_em_iters iterations) from per-speaker sums / counts and
 *                      the scatter statistics of the same rows; mean[dim], transform[dim][dim], psi[dim] (descending);
 *                      n_floored (optional) = between-class eigenvalues floored at zero.
 *   xv_plda_adapt      host only: ivector-adapt-plda (PldaUnsupervisedAdaptor::UpdatePlda) from the statistics of n >= 1
 *                      unlabelled vectors, m[dim] = sum x and v[dim][dim] = sum x x^T (xv_scatter_stats with one segment
 *                      that lists every row: sums and s_tot), the model (mean, transform, psi >= 0) and the three scales
 *                      (Kaldi's defaults 1.0, 0.3, 0.7); mean_out[dim], transform_out[dim][dim], psi_out[dim] (descending);
 *                      s_out (optional, [dim]) = eigenvalues of the adaptation covariance in the space where the model's
 *                      total covariance is I, descending.
 * The device entries fail with XV_ERR_DEVICE when no gfx950 device is usable.
 * Score normalisation on top of xv_plda_score (all pairs, top-N statistics) is declared in xvec_hip_asnorm.h. */
xv_status xv_scatter_stats(int device, const float* x, int32_t n, int32_t dim, const int32_t* seg_off, const int32_t* idx,
                           int32_t n_seg, double* s_tot, double* sums, double* s_bet, float* device_ms);
xv_status xv_plda_transform(int device, const float* x, int32_t n, int32_t dim, const double* transform, const double* offset,
                            const double* psi, const double* num, int32_t normalize, int32_t simple, float* y, double* scale,
                            float* device_ms);
xv_status xv_plda_score(int device, const float* u, const double* num_u, int32_t n_u, const float* v, int32_t n_v, int32_t dim,
                        const double* psi, const int32_t* trials, int64_t n_trials, double* scores, float* device_ms);
xv_status xv_lda_estimate(int32_t dim, int64_t n, const double* s_tot, const double* s_bet, const float* mean,
                          double total_covariance_factor, double covariance_floor, int32_t lda_dim, float* out, int32_t* n_floored);
xv_status xv_plda_estimate(int32_t dim, int32_t n_spk, const double* sums, const int32_t* counts, const double* s_tot,
                           const double* s_bet, int32_t num_em_iters, double* mean, double* transform, double* psi,
                           int32_t* n_floored);
xv_status xv_plda_adapt(int32_t dim, int64_t n, const double* m, const double* v, const double* mean, const double* transform,
                        const double* psi, double mean_diff_scale, double within_covar_scale, double between_covar_scale,
                        double* mean_out, double* transform_out, double* psi_out, double* s_out);

/* ---- feature stage (stage 1 of egs/sre/v2/run_sre10.sh:78-90: compute-mfcc-feats, compute-vad) -------------------
 * Waveform to MFCC and MFCC to energy-VAD decisions on the device, behind host buffers.  Semantics are Kaldi's
 * (option names and defaults of compute-mfcc-feats / compute-vad); fp32 arithmetic.  A result depends on the utterance
 * and the options, never on the batch: an utterance computed alone and inside any batch gives the same bytes.
 * window_type: 0 povey, 1 hamming, 2 hanning, 3 rectangular, 4 blackman.  Not built (XV_ERR_ARG): VTLN, HTK
 * compatibility, round_to_power_of_two == 0, resampling.
 *   xv_mfcc_options_default  Kaldi's defaults (16 kHz, 25/10 ms, povey, dither 1.0, 23 mel bins, 13 ceps, lifter 22).
 *   xv_mfcc_num_frames       host only: frames Kaldi extracts from n_samples samples (snip_edges true: 1 + (n - L)/S for
 *                            n >= L, else 0; false: (n + S/2)/S); -1 with xv_last_error() for unusable options.
 *   xv_mfcc_utt_seed         host only: the 64-bit hash of an utterance key that keys the dither generator.
 *   xv_mfcc_compute          samples: fp32 in Kaldi's unscaled range (+-32768), utterance u = samples[sample_offsets[u] ..
 *                            sample_offsets[u+1]); utt_seeds [n_utts] may be NULL when dither == 0 (else XV_ERR_ARG).
 *                            out_row_offsets [n_utts + 1] is written (frame offsets); out receives
 *                            out_row_offsets[n_utts] * num_ceps floats - size it with xv_mfcc_num_frames.  Dither is drawn
 *                            from a counter-based generator keyed by (seed, frame, sample): reproducible, and the same in
 *                            any job, shard or batch; it matches Kaldi's rand()-driven dither in distribution only.
 *   xv_mfcc_compute_i16      the same for 16-bit PCM (converted on the device; the same bytes out).
 *   xv_vad_energy            Kaldi's ComputeVadEnergy on feats [row_offsets[n_utts]][dim] (column 0 = log energy):
 *                            out[row] = 1.0 / 0.0 per frame.  The utterance mean is summed in a fixed order in fp64.
 *   xv_wave_read             host only: reads a RIFF/WAVE (16-bit PCM) from an rxfilename (file or "cmd |"), picks a channel
 *                            as compute-mfcc-feats --channel does (-1: mono as is, else channel 0); *samples is malloc'ed
 *                            [*n] int16, released with xv_wave_free.
 *   xv_mfcc_kernel_time      for tools/bench_mfcc.py: runs the int16 batch reps times on one set of device buffers and returns the
 *                            shortest kernel time between two events (ms), copies excluded.
 * The device entries fail with XV_ERR_DEVICE when no gfx950 device is usable. */
typedef struct {
  float sample_frequency, frame_length_ms, frame_shift_ms, dither, preemphasis_coefficient, blackman_coeff;
  int32_t remove_dc_offset, window_type, round_to_power_of_two, snip_edges;
  int32_t num_mel_bins;
  float low_freq, high_freq;
  int32_t num_ceps;
  float cepstral_lifter;
  int32_t use_energy, raw_energy;
  float energy_floor;
} xv_mfcc_options;
typedef struct {
  float vad_energy_threshold, vad_energy_mean_scale, vad_proportion_threshold;
  int32_t vad_frames_context;
} xv_vad_options;
void xv_mfcc_options_default(xv_mfcc_options* opts);
int64_t xv_mfcc_num_frames(const xv_mfcc_options* opts, int64_t n_samples);
uint64_t xv_mfcc_utt_seed(const char* key);
xv_status xv_mfcc_compute(int device, const xv_mfcc_options* opts, const float* samples, const int64_t* sample_offsets,
                          int32_t n_utts, const uint64_t* utt_seeds, float* out, int32_t* out_row_offsets);
xv_status xv_mfcc_compute_i16(int device, const xv_mfcc_options* opts, const int16_t* samples, const int64_t* sample_offsets,
                              int32_t n_utts, const uint64_t* utt_seeds, float* out, int32_t* out_row_offsets);
xv_status xv_mfcc_kernel_time(int device, const xv_mfcc_options* opts, const int16_t* samples, const int64_t* sample_offsets,
                              int32_t n_utts, int32_t reps, float* kernel_ms);
xv_status xv_vad_energy(int device, const xv_vad_options* vad_opts, const float* feats, const int32_t* row_offsets,
                        int32_t n_utts, int32_t dim, float* out);
xv_status xv_wave_read(const char* rxfilename, int32_t channel, int32_t* rate, int16_t** samples, int64_t* n);
void xv_wave_free(int16_t* samples);

/* ---- augmentation stage (stage 2 of egs/sre/v2/run_sre10.sh:92-159: wav-reverberate) -------------------------------
 * Convolution with a room impulse response, additive noises at given SNRs and start times, normalisation, shift, trim or
 * repetition and the conversion to 16-bit samples, on the device for a ragged batch.  Semantics are Kaldi's wav-reverberate for
 * one output channel (csrc/reverb.h restates them); fp32 signals, fp64 power sums in a fixed order.  An utterance's output
 * depends on the utterance alone, never on the batch.
 *   xv_reverb_options_default  Kaldi's defaults: shift_output 1, normalize_output 1, duration 0, volume 0, channels 0.
 *   xv_reverb_output_length    host only: samples written for an input of n samples and a RIR of rir_len taps (0: none).
 *   xv_wav_reverberate         samples: int16 (samples_are_i16 != 0) or fp32 in the 16-bit range, utterance u =
 *                              [sample_offsets[u], sample_offsets[u+1]), all at sample_rate.  rirs / noises: fp32 as read from
 *                              their files (not scaled), ragged by rir_offsets [n_rirs + 1] / noise_offsets [n_noises + 1].
 *                              utt_rir [n_utts]: index of the utterance's RIR or -1 (NULL: none anywhere; utterances that name
 *                              the same index share its spectra).  The additive signals of utterance u are entries
 *                              [utt_add_offsets[u], utt_add_offsets[u+1]) of add_noise (index into the noises), add_snr (dB)
 *                              and add_start (seconds); utt_add_offsets NULL: none.  out_offsets [n_utts + 1] is written;
 *                              out_f32 receives out_offsets[n_utts] floats, the signal before quantisation - size it with
 *                              xv_reverb_output_length; out_i16 (may be NULL) the samples as a wave file holds them (truncated
 *                              toward zero, saturated) and clipped (may be NULL) [n_utts] how many were saturated.  The
 *                              channel fields of the options are for the readers of files and are not looked at here.
 *   xv_reverb_kernel_time      for tools/bench_reverb.py: the same call reps times, returns the shortest sum of the kernels'
 *                              times between events (ms), copies excluded.
 *   xv_recognize_wav_pipeline  host only: whether a wav.scp entry is a pipe that compute-mfcc-feats takes over instead of running
 *                              it (last stage wav-reverberate with only its own options, reading "-" or one file, writing
 *                              "-"; one level of nesting inside the additive signals; csrc/fuse_wav.h); *found = 0 / 1 and,
 *                              when found, description receives "name=value" lines: source, impulse-response, the options
 *                              and additive[i].snr / .start / .rx or the nested element's fields.
 *   xv_wave_write              host only: writes one channel as RIFF/WAVE, 16-bit PCM, to a wxfilename (file, "-" or "| cmd"),
 *                              fp32 samples truncated toward zero and saturated as above; *clipped (may be NULL) the count. */
typedef struct {
  int32_t shift_output, normalize_output;
  float duration, volume;
  int32_t input_wave_channel, rir_channel, noise_channel;
} xv_reverb_options;
void xv_reverb_options_default(xv_reverb_options* opts);
int64_t xv_reverb_output_length(const xv_reverb_options* opts, float sample_rate, int64_t n_samples, int64_t rir_len);
xv_status xv_wav_reverberate(int device, const xv_reverb_options* opts, float sample_rate, const void* samples,
                             int32_t samples_are_i16, const int64_t* sample_offsets, int32_t n_utts, const float* rirs,
                             const int64_t* rir_offsets, int32_t n_rirs, const int32_t* utt_rir, const float* noises,
                             const int64_t* noise_offsets, int32_t n_noises, const int32_t* utt_add_offsets,
                             const int32_t* add_noise, const float* add_snr, const float* add_start, int64_t* out_offsets,
                             float* out_f32, int16_t* out_i16, int64_t* clipped);
xv_status xv_reverb_kernel_time(int device, const xv_reverb_options* opts, float sample_rate, const void* samples,
                                int32_t samples_are_i16, const int64_t* sample_offsets, int32_t n_utts, const float* rirs,
                                const int64_t* rir_offsets, int32_t n_rirs, const int32_t* utt_rir, const float* noises,
                                const int64_t* noise_offsets, int32_t n_noises, const int32_t* utt_add_offsets,
                                const int32_t* add_noise, const float* add_snr, const float* add_start, int32_t reps,
                                float* kernel_ms);
xv_status xv_recognize_wav_pipeline(const char* rxfilename, int32_t* found, char* description, size_t description_cap);
xv_status xv_wave_write(const char* wxfilename, int32_t rate, const float* samples, int64_t n, int64_t* clipped);

/* ---- kernel-level entry (unit tests of the HIP GEMM against a plain fp32 reference) ------------------- */
typedef struct {
  const void* hi;   /* device plane (bf16 / fp16) at logical row 0 */
  const void* lo;   /* residual plane (XV_PREC_BF16X3 / XV_PREC_FP16X3 only) */
  int32_t ld;       /* leading dimension in elements */
  int32_t row_shift;
  int32_t k_len;    /* multiple of 32 */
  const void* gmax; /* XV_PREC_FP16MX: device uint32 [rows/16], float bits of max |x| per 16-row group of this plane */
  /* XV_PREC_FP16MX2: 4-bit image of (activation - hi), [rows][ld / 2 bytes], and its E8M0 scales [rows][ld / 64 rounded up to a multiple of 4] (what
   * epilogue 0 of XV_PREC_FP16MX2 / XV_PREC_FP16X3E / XV_PREC_FP16MXE wrote to out_lo4 / out_lo4_scale), both at logical row 0 */
  const void* lo4; const void* lo4_scale;
} xv_seg_desc;
typedef struct {
  int32_t precision, epilogue; /* epilogue: 0 planes out, 1 fp32 out, 2 per-16-row (sum, sumsq) partials */
  int32_t nseg;
  xv_seg_desc seg[8];
  const void* w_hi; const void* w_lo; int32_t ldw;
  int32_t rows;     /* multiple of 128 */
  int32_t n_pad;    /* multiple of 128 */
  const float* bias; const float* scale; const float* offset;
  int32_t relu, bn;
  void* out_hi; void* out_lo; int32_t ldo;
  float* out_f32; int32_t ldf; int32_t m_valid;
  float* partial; int32_t ldp; const int8_t* grp_range;
  void* hip_stream;
  /* XV_PREC_FP16MX: e2m1 residual plane [n_pad][ldw4 bytes] in K-walk order + its E8M0 scales, one per row, block of four K
   * steps and lane group, in the staging order of this epilogue (xv_tile_mx_scales; see kernels.h);
   * gmax_out (epilogue 0, any precision): device uint32 [rows/16], receives the group maxima of the output plane */
  const void* w4; int32_t ldw4; const void* w4_scale;
  void* gmax_out;
  /* XV_PREC_FP16MX2: 4-bit image of the weights for the second K walk (xv_pack_mx_weights) + scales in staging order;
   * out_lo4 / out_lo4_scale (epilogue 0 of XV_PREC_FP16MX2 / XV_PREC_FP16X3E / XV_PREC_FP16MXE): see xv_seg_desc */
  const void* w4b; int32_t ldw4b; const void* w4b_scale;
  void* out_lo4; void* out_lo4_scale;
  /* != 0: run tdnn_gemm_kernel_p8 (256 x 256 tiles, K tiles of 64 columns; XV_PREC_FP16, XV_PREC_FP16MX and XV_PREC_FP16MX2,
   * epilogues 0 and 2; rows and n_pad multiples of 256).  Its K walk is group -> 64-column chunk -> offset: w4 / w4_scale must
   * come from xv_pack_mx_residual64 (and, XV_PREC_FP16MX2, w4b / w4b_scale from xv_pack_mx_weights64 with ldw4b = 2 * ldw).  A layer runs this kernel for every launch of a mode or for none (its sums are formed in
   * another order than the 32-column kernels'). */
  int32_t p8;
  /* epilogue 0 with gmax_out: device int8 [rows/16][2], first / last (exclusive) row of every 16-row group that counts for its
   * maximum (NULL: every row) */
  const int8_t* out_range;
  /* > 1: split-K (XV_PREC_BF16X3 .. XV_PREC_FP16X3, epilogues 0 and 1, not p8): the K steps are divided over slices by the
   * engine's rule (at least 4 steps per slice, at most 24 slices), whose raw sums a second kernel adds in slice order.  The value
   * must be the number of slices that rule gives for this K (XV_ERR_ARG otherwise); the entry owns the workspace.  0 / 1: off */
  int32_t ksplit;
} xv_gemm_desc;
/* Host helper for the test above: packs the e2m1 residual plane of one weight matrix exactly like xv_model_pack does
 * (w, w_hi_f16: [n_pad][k_len] row-major, k_len = sum of the segments' k_len; seg_src[j] equal = same source plane).
 * w4 receives n_pad * (k_len / 128 * 64) bytes, w4_scale n_pad * (k_len / 32) bytes.  XV_ERR_ARG when the walk has a group that is
 * not a multiple of four steps. */
xv_status xv_pack_mx_residual(const float* w, const uint16_t* w_hi_f16, int32_t n_pad, int32_t nseg,
                              const int32_t* seg_src, const int32_t* seg_shift, const int32_t* seg_klen, uint8_t* w4,
                              uint8_t* w4_scale);
/* the same in the K-walk order of tdnn_gemm_kernel_p8 (xv_gemm_desc.p8) */
xv_status xv_pack_mx_residual64(const float* w, const uint16_t* w_hi_f16, int32_t n_pad, int32_t nseg, const int32_t* seg_src,
                                const int32_t* seg_shift, const int32_t* seg_klen, uint8_t* w4, uint8_t* w4_scale);
/* XV_PREC_FP16MX2: the 4-bit image of the weights for the second K walk (w: [n_pad][k_len], the values of the fp16 planes'
 * domain; every k_len a multiple of 128): w4b receives n_pad * (k_len / 128 * 64) bytes, w4b_scale n_pad * (k_len / 32)
 * bytes in natural order (tile them with xv_tile_mx_scales). */
xv_status xv_pack_mx_weights(const float* w, int32_t n_pad, int32_t nseg, const int32_t* seg_src, const int32_t* seg_shift,
                             const int32_t* seg_klen, uint8_t* w4b, uint8_t* w4b_scale);
/* the same in the order of tdnn_gemm_kernel_p8's second walk (tiles of 256 columns: every k_len a multiple of 256), rows of
 * k_len * 2 bytes - the pitch of the fp16 plane, which is what xv_gemm_desc.ldw4b must then say: w4b receives n_pad * k_len * 2 bytes */
xv_status xv_pack_mx_weights64(const float* w, int32_t n_pad, int32_t nseg, const int32_t* seg_src, const int32_t* seg_shift,
                               const int32_t* seg_klen, uint8_t* w4b, uint8_t* w4b_scale);
/* natural[n_pad][k_len / 32] (what xv_pack_mx_residual / xv_pack_mx_weights wrote) -> the order the kernels stage the scales in for the given
 * epilogue (xv_gemm_desc.epilogue): n_pad * (k_len / 32) bytes.  n_pad must be a multiple of 128. */
xv_status xv_tile_mx_scales(const uint8_t* natural, int32_t n_pad, int32_t k_len, int32_t epilogue, uint8_t* tiled);
xv_status xv_kernel_tdnn_gemm(const xv_gemm_desc* d);
/* Name of the kernel instantiation the calling thread's last xv_kernel_tdnn_gemm launched, e.g. "tdnn_gemm_kernel_sk<fp16x2,act,8>"
 * ("tdnn_gemm_kernel<bf16x3,splitk>" for a split-K launch; "" before the first one).  Valid on the calling thread until its next launch. */
const char* xv_last_gemm_kernel(void);
/* What xv_kernel_tdnn_gemm would launch for a descriptor, without launching: the launch is decided by one host function
 * (csrc/gemm_plan.h) that this entry asks.  No device is needed, and the descriptor's pointers are only looked at for being null
 * or equal (any distinct non-null values will do).  cus > 0: a device of that many CUs under the default XVEC_DEBUG knobs;
 * cus <= 0: the current device and this process's knobs.  A launch the entry would refuse gives XV_OK with refused = 1. */
typedef struct {
  int32_t ld, ksteps, nshift, shift0, dstep, wcol0, wstride, ld4s;   /* the scalar fields of a K-walk group (csrc/kernels.h, Grp) */
} xv_gemm_plan_group;
typedef struct {
  int32_t refused;
  char kernel[96];                /* as xv_last_gemm_kernel spells it; "" when refused */
  int32_t grid_x, grid_y, block, lds_bytes;
  int32_t mf;                     /* stream-K: 16-row fragments per wave (4 or 8), else 0 */
  int32_t lanes, groups_per_xcd;  /* persistent kernels (stream-K, p8): column lanes, workgroup groups per XCD block and lane */
  int32_t sk_mtiles, p8_ktiles, p8_ktiles_lo, p8_whole, stagger_units;
  int64_t workspace_bytes;        /* stream-K exchange workspace */
  int32_t ngrp, ngrp_lo, lo_ksteps;   /* the K walk (not planned for split-K): grp[0 .. ngrp) the groups of the first walk, */
  xv_gemm_plan_group grp[16];         /* grp[ngrp .. ngrp + ngrp_lo) of the second (XV_PREC_FP16MX2) */
} xv_gemm_plan;
xv_status xv_plan_gemm(const xv_gemm_desc* d, int32_t cus, xv_gemm_plan* out);
/* the same under an explicit policy: the CU count and the knobs gemm_variant, sk_mf, sk_lanes, gemm_stagger (csrc/knobs.h) */
xv_status xv_plan_gemm_policy(const xv_gemm_desc* d, int32_t cus, int32_t variant, int32_t sk_mf, int32_t sk_lanes,
                              int32_t stagger_pct, xv_gemm_plan* out);

/* ---- compressed feature matrices (copy-feats --compress=true) and stage 3 of the recipes, without a model context ------------
 * Kaldi's CompressedMatrix as csrc/compress.h restates it.  method: 1 automatic ("CM" when rows > 8, else "CM2"), 2 "CM", 3 "CM2",
 * 5 "CM3"; the fixed-range methods 4, 6 and 7 are XV_ERR_ARG.  An object is what follows the "CM " / "CM2 " / "CM3 " token. */
/* host only: the size of the object of a rows x cols matrix and its token (a static string) */
xv_status xv_compressed_size(int32_t rows, int32_t cols, int32_t method, size_t* nbytes, const char** format);
/* host buffers, blocking: the n matrices feats[row_off[u] .. row_off[u + 1])[cols] (row-major, packed) are compressed on the device;
 * object u is written to out_bytes + out_off[u], out_off[n + 1] is filled by the call (objects follow each other without gaps;
 * size the buffer with xv_compressed_size).  nonfinite_flags[u] != 0 (may be NULL): the matrix holds a NaN or an infinity, or
 * its range is not finite, and its object means nothing - write the floats instead.  A matrix's bytes depend on the matrix and
 * the method only. */
xv_status xv_compress_matrices(int device, const float* feats, const int32_t* row_off, int32_t n, int32_t cols, int32_t method,
                               uint8_t* out_bytes, int64_t* out_off, int32_t* nonfinite_flags);
/* the kernels' time of one such call in ms: the best of reps runs after one that warms up */
xv_status xv_compress_kernel_time(int device, const float* feats, const int32_t* row_off, int32_t n, int32_t cols, int32_t method,
                                  int32_t reps, float* kernel_ms);
/* apply-cmvn-sliding --norm-vars=false: the kernels of xv_frontend_cmvn_select with every frame kept (cols <= 64); out has the
 * shape of raw.  raw_off[0] must be 0. */
xv_status xv_cmvn_sliding(int device, const float* raw, const int32_t* raw_off, int32_t n, int32_t cols, int32_t cmn_window,
                          int32_t min_cmn_window, int32_t center, float* out);

/* ---- per-speaker cepstral mean and variance normalisation (compute-cmvn-stats / apply-cmvn), without a model context ----------
 * Kaldi's transform/cmvn.cc as csrc/cmvn.h restates it. */
/* host buffers, blocking: Kaldi's statistics of the n_utts matrices feats[row_off[u] .. row_off[u + 1])[cols] (row-major, packed;
 * row_off[0] = 0), summed on the device in fp64: stats[u] = double[2][cols + 1], row 0 the column sums and the frame count, row 1
 * the sums of squares and 0.  The order of every sum depends on the matrix's shape only: a matrix's statistics are the same bits
 * in whatever batch it is.  device_ms (may be NULL): the kernels' time. */
xv_status xv_cmvn_stats(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, double* stats,
                        float* device_ms);
/* host only: one statistics matrix -> float norm[2][cols], row 0 the offset and row 1 the scale of out = x * scale + offset.
 * Computed in fp64, stored as float.  A count below 1 is XV_ERR_IO ("Insufficient stats ..."); norm_vars without norm_means is
 * XV_ERR_ARG.  skip_dims [n_skip]: columns left as they are.  num_floored (may be NULL): variances floored at 1e-20. */
xv_status xv_cmvn_norm(const double* stats, int32_t cols, int32_t norm_means, int32_t norm_vars, int32_t reverse,
                       const int32_t* skip_dims, int32_t n_skip, float* norm, int32_t* num_floored);
/* host buffers, blocking: out[r][d] = feats[r][d] * scale + offset on the device, in fp32 with the product and the sum each rounded
 * on their own; matrix u takes norm utt_norm[u] (>= 0) of norms[..][2][cols].  out has the shape of feats. */
xv_status xv_cmvn_apply(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, const float* norms,
                        const int32_t* utt_norm, float* out);
/* host buffers, blocking: the same map behind a row selection, as one launch: out[i][d] = feats[sel_row[i]][d] * scale + offset with
 * norm utt_norm[sel_utt[i]] of norms[n_norms][2][cols] - bit for bit the rows sel_row of what xv_cmvn_apply writes.  sel_row:
 * absolute rows of feats, each inside utterance sel_utt[i] (the layout of xv_frontend_cmvn_select); an utterance without a selected
 * row may have utt_norm = -1.  Any cols >= 1.  out: [n_out][cols].  A table that does not check out is XV_ERR_IO. */
xv_status xv_cmvn_apply_select(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, const float* norms,
                               int32_t n_norms, const int32_t* utt_norm, const int32_t* sel_row, const int32_t* sel_utt, int32_t n_out,
                               float* out);
/* host only: whether a feature rspecifier is the per-speaker pipeline nnet3-compute runs on the device instead of as commands
 * ("ark[,letters]:apply-cmvn [--norm-means=B] [--norm-vars=B] [--utt2spk=ark:FILE] <stats> <feats> ark:- | [select-voiced-frames
 * ark:- <vad> ark:- |]", csrc/fuse_pipe.h); *found = 0 / 1 and, when found, description receives "name=value" lines: stats,
 * stats-is-table, feats, vad, utt2spk, norm-means, norm-vars. */
xv_status xv_recognize_cmvn_pipeline(const char* rspecifier, int32_t* found, char* description, size_t description_cap);
/* the kernels' times of one statistics call and one application in ms: the best of reps runs after one that warms up */
xv_status xv_cmvn_kernel_time(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, int32_t reps,
                              float* stats_ms, float* apply_ms);

/* ---- the GMM-UBM stage of the i-vector baseline (add-deltas, gmm-gselect, fgmm-global-gselect-to-post), without a model context
 * Semantics: csrc/ubm.h.  Everything on the device is fp32 with a summation order that depends on the frame and the model alone: a
 * frame's results are the same bits in whatever batch it is.  Limits: n <= 64 selected Gaussians, dimension <= 96. */
typedef struct xv_ubm xv_ubm;
/* host buffers, blocking: out[r] = the (order + 1) blocks of D = (truncate > 0 ? truncate : cols) columns, utterance by utterance
 * (row_off[0] = 0).  fp32, every product and every sum rounded on its own.  device_ms may be NULL. */
xv_status xv_add_deltas(int device, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t cols, int32_t order,
                        int32_t window, int32_t truncate, float* out, float* device_ms);
/* A model is uploaded once per process and device and used through its handle.  Host arrays: gconsts [G]; diagonal:
 * means_invvars and inv_vars [G][D]; full: means_invcovars [G][D] and inv_covars [G][D (D + 1) / 2], the packed lower triangles. */
xv_status xv_ubm_diag_create(int device, int32_t num_gauss, int32_t dim, const float* gconsts, const float* means_invvars,
                             const float* inv_vars, xv_ubm** out);
xv_status xv_ubm_full_create(int device, int32_t num_gauss, int32_t dim, const float* gconsts, const float* means_invcovars,
                             const float* inv_covars, xv_ubm** out);
void xv_ubm_destroy(xv_ubm* m);
/* the n best Gaussians of a diagonal model per frame, best first: idx [rows][n]; loglikes (may be NULL) the same shape.
 * n above 64 or above the model's size is XV_ERR_IO and names the limit. */
xv_status xv_ubm_gselect(const xv_ubm* diag, const float* feats, const int32_t* row_off, int32_t n_utts, int32_t n, int32_t* idx,
                         float* loglikes, float* device_ms);
/* posteriors of a full model over the selected Gaussians gselect [rows][n]: count [rows]; idx and post [rows][n], of which the
 * first count[t] entries of frame t are set (selection order, zeros dropped) and the rest are -1 / 0.  loglikes ([rows][n], before
 * the softmax) and logsum ([rows]) may be NULL.  device_ms3 (may be NULL): the times of the sort, the scores and the softmax. */
xv_status xv_ubm_post(const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* gselect, int32_t n,
                      float min_post, int32_t* count, int32_t* idx, float* post, float* loglikes, float* logsum, float* device_ms3);
/* host only (fp64): a full model to its diagonal image; gconsts_out [G], means_invvars_out and inv_vars_out [G][D] */
xv_status xv_fgmm_to_gmm(int32_t num_gauss, int32_t dim, const float* weights, const float* means_invcovars, const float* inv_covars,
                         float* gconsts_out, float* means_invvars_out, float* inv_vars_out);
/* host only (fp64, stored as float): the gconsts the tools recompute after they read a full model (csrc/ubm.h); a component
 * whose inverse covariance is not positive definite gets -infinity.  num_bad (may be NULL): how many those are. */
xv_status xv_fgmm_gconsts(int32_t num_gauss, int32_t dim, const float* weights, const float* means_invcovars, const float* inv_covars,
                          float* gconsts_out, int32_t* num_bad);
/* the kernels' times in ms, the best of reps runs after one that warms up: ms5 = {deltas (order 2, window 3 on the first dim / 3
 * columns; 0 if dim is no multiple of 3), selection, sort, full-covariance scores, softmax}.  The two models share their
 * dimension, which is the features'; 1 <= n <= 64. */
xv_status xv_ubm_kernel_time(const xv_ubm* diag, const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts,
                             int32_t n, float min_post, int32_t reps, float* ms5);

/* ---- the GMM classifiers (fgmm-gselect --gselect=, fgmm-global-get-frame-likes, compute-vad-from-frame-likes, merge-vads;
 * sid/gender_id.sh:88-118, sid/music_id.sh:73-104, sid/compute_vad_decision_gmm.sh:91-127).  Semantics: csrc/gmm_classify.h.
 * Limits: n_in <= 64 preselected Gaussians, dimension <= 96, dense frame likelihoods only for models of at most 64 components. */
/* second-stage selection by a full model: preselect [rows][n_in], every entry in [0, G); idx and loglikes (may be NULL) are
 * [rows][min(n_out, n_in)], best first (score descending, then Gaussian ascending, then slot ascending).  The scores are bit for
 * bit xv_ubm_post's loglikes.  n_in above 64 is XV_ERR_IO and names the limit.  device_ms3 (may be NULL): sort, scores, rerank. */
xv_status xv_ubm_full_gselect(const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* preselect,
                              int32_t n_in, int32_t n_out, int32_t* idx, float* loglikes, float* device_ms3);
/* likes [rows]: the log-sum-exp of a full model's scores over gselect [rows][n], bit for bit xv_ubm_post's logsum at min_post = 0.
 * gselect NULL: every component is scored (n is ignored); a model of more than 64 components is then XV_ERR_IO and names the
 * limit.  device_ms3 (may be NULL): sort, scores, softmax. */
xv_status xv_ubm_frame_likes(const xv_ubm* full, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* gselect, int32_t n,
                             float* likes, float* device_ms3);
/* host only: out[t] = the first class j that maximises likes[j][t] + log(priors[j]), as map[j] if map is given.  likes: n_classes
 * arrays of rows floats; priors (NULL: all 1) and map (NULL: the class itself): [n_classes].  A prior <= 0 is XV_ERR_IO. */
xv_status xv_vad_from_frame_likes(int32_t n_classes, const float* const* likes, int64_t rows, const float* priors, const int32_t* map, float* out);
/* host only: n_triples = 0: out[t] = 1 iff a[t] and b[t] are 1, else 0.  Otherwise map_triples [n_triples][3] sends the pair
 * (a[t], b[t]) to the third entry; a pair that is not in the map is XV_ERR_IO and is named. */
xv_status xv_merge_vads(const float* a, const float* b, int64_t rows, const int32_t* map_triples, int32_t n_triples, float* out);

/* ---- full-covariance UBM training (fgmm-global-acc-stats, fgmm-global-est; sid/train_full_ubm.sh:69-118), without a model context.
 * Semantics: csrc/ubm_train.h.  The accumulators are fp64 on the device; no floating-point value goes through an atomic, and what a
 * call adds is a function of the call's frames and pairs alone.  Limits: dimension <= 96, n <= 64 selected Gaussians. */
typedef struct xv_fgmm_acc xv_fgmm_acc;
/* update_flags: letters of "mvw" (v implies m, m implies w, as Kaldi augments them).  The accumulators start at zero. */
xv_status xv_fgmm_acc_create(int device, int32_t num_gauss, int32_t dim, const char* update_flags, xv_fgmm_acc** out);
void xv_fgmm_acc_destroy(xv_fgmm_acc* a);
/* host buffers, blocking, one call with no internal blocking: feats [rows][dim]; frame t has the pairs post_off[t] .. post_off[t + 1]
 * (post_off has rows + 1 entries) of post_idx (Gaussian, in [0, G): anything else is XV_ERR_IO before anything is uploaded) and
 * post_w.  A pair whose weight is 0 adds nothing. */
xv_status xv_fgmm_acc_add(xv_fgmm_acc* a, const float* feats, int32_t rows, const int32_t* post_off, const int32_t* post_idx,
                          const float* post_w);
/* the fused E-step: the posteriors of xv_ubm_post (min_post = 0) over gselect [rows][n] are accumulated without leaving the device;
 * logsum [rows] comes back.  The model must have the accumulators' shape and device. */
xv_status xv_fgmm_acc_add_gselect(xv_fgmm_acc* a, const xv_ubm* full, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  float* logsum);
/* downloads occ [G], mean [G][D] and cov [G][D (D + 1) / 2] (packed lower triangles); any of them may be NULL */
xv_status xv_fgmm_acc_get(const xv_fgmm_acc* a, double* occ, double* mean, double* cov);
/* host only (fp64): the M-step of fgmm-global-est on host arrays.  acc_flags: the accumulators' letters; update_flags must be among
 * them (after augmentation).  weights [G], means_invcovars [G][D] and inv_covars [G][D (D + 1) / 2] are updated in place, the
 * Gaussians that survive moved to the front; gconsts [G] is written.  *num_gauss_out: how many survive; removed [G]: the first
 * G - *num_gauss_out entries are the indices taken out.  floored2 = {eigenvalues floored, Gaussians they belong to}; objf3 = {the
 * objective before, after, the sum of occ}.  removed, floored2 and objf3 may be NULL. */
xv_status xv_fgmm_est(int32_t num_gauss, int32_t dim, const char* acc_flags, const double* occ, const double* mean, const double* cov,
                      const char* update_flags, double min_gaussian_weight, double min_gaussian_occupancy, double variance_floor,
                      double max_condition, int32_t remove_low_count_gaussians, float* weights, float* means_invcovars, float* inv_covars,
                      float* gconsts, int32_t* num_gauss_out, int32_t* removed, int32_t* floored2, double* objf3);
/* the kernels' times in ms of one fused call, the best of reps runs after one that warms up: ms4 = {sort, full-covariance scores,
 * softmax, fgmm_acc (its work-item pass included)}.  Every run adds the call's statistics to the accumulators. */
xv_status xv_fgmm_acc_kernel_time(xv_fgmm_acc* a, const xv_ubm* full, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  int32_t reps, float* ms4);

/* ---- the phonetic i-vector path (logprob-to-post, fgmm-global-init-from-accs; sid/extract_post_nnet3.sh:85-91,
 * sid/init_full_ubm_from_nnet3.sh:118-136), without a model context.  Semantics: csrc/post.h. */
/* host buffers, blocking: logprobs [row_off[n_utts]][cols] packed, utterance by utterance (row_off[0] = 0); keys [n_utts] are the
 * utterance keys that key the random pruning (may be NULL with random_prune == 0 or min_post <= 0).  frame_budget: rows per launch,
 * <= 0 for the default; the result does not depend on it.  pair_off [rows + 1] is always written: row r has the pairs
 * pair_off[r] .. pair_off[r + 1], columns ascending.  *need is their number; idx and post (room for `capacity` pairs each, may be
 * NULL with capacity 0) are written only if *need <= capacity: otherwise call again with that much room.  num_nan (may be NULL):
 * the NaN inputs that were dropped.  device_ms3 (may be NULL): the times of the count, the scan and the write kernels. */
xv_status xv_logprob_to_post(int device, const float* logprobs, const int32_t* row_off, int32_t n_utts, int32_t cols, const char* const* keys,
                             float min_post, int32_t random_prune, int32_t frame_budget, int64_t capacity, int64_t* pair_off, int32_t* idx,
                             float* post, int64_t* need, int64_t* num_nan, float* device_ms3);
/* the kernels' times in ms of one utterance of rows x cols, the best of reps runs after one that warms up: ms4 = {count, scan, write,
 * a device-to-device copy of the input}.  The copy reads and writes the input once: its time is what two reads of the input cost at
 * the copy bandwidth of the same run, the floor of the count and write passes together. */
xv_status xv_logprob_to_post_kernel_time(int device, const float* logprobs, int32_t rows, int32_t cols, const char* key, float min_post,
                                         int32_t random_prune, int32_t reps, float* ms4);
/* host only (fp64): a full-covariance model from accumulators that carry m, v and w: occ [G], mean [G][D], cov [G][D (D + 1) / 2].
 * weights_out [G], means_invcovars_out [G][D], inv_covars_out [G][D (D + 1) / 2] and gconsts_out [G] get the Gaussians that
 * survive, at the front; *num_gauss_out how many.  removed [G] (may be NULL): the first G - *num_gauss_out entries are the indices
 * taken out.  With remove_low_count_gaussians == 0 a bad Gaussian is XV_ERR_IO and names it.  num_bad_gconsts may be NULL.
 * inv_covars_f64 (may be NULL): [G][D (D + 1) / 2], the inverse covariance of every Gaussian as given (none moved; zeros for one
 * taken out) before it is rounded to float. */
xv_status xv_fgmm_init_from_accs(int32_t num_gauss, int32_t dim, const double* occ, const double* mean, const double* cov,
                                 int32_t remove_low_count_gaussians, float* weights_out, float* means_invcovars_out, float* inv_covars_out,
                                 float* gconsts_out, int32_t* num_gauss_out, int32_t* removed, int32_t* num_bad_gconsts, double* inv_covars_f64);

/* ---- diagonal UBM training (gmm-global-init-from-feats, gmm-global-acc-stats, gmm-global-est; sid/train_diag_ubm.sh:105-137), without
 * a model context.  Semantics: csrc/dubm_train.h.  The accumulators are fp64 on the device; no floating-point value goes through an
 * atomic, and what a call adds is a function of the call's frames, pairs and model alone.  A (frame, Gaussian) score is bit for bit
 * the one xv_ubm_gselect ranks.  Limits: dimension <= 96, n <= 64 selected Gaussians. */
typedef struct xv_dgmm_acc xv_dgmm_acc;
/* update_flags: letters of "mvw" (v implies m, m implies w).  The accumulators start at zero. */
xv_status xv_dgmm_acc_create(int device, int32_t num_gauss, int32_t dim, const char* update_flags, xv_dgmm_acc** out);
void xv_dgmm_acc_destroy(xv_dgmm_acc* a);
/* the caller's sparse pairs through the accumulator kernels alone; the arguments of xv_fgmm_acc_add */
xv_status xv_dgmm_acc_add(xv_dgmm_acc* a, const float* feats, int32_t rows, const int32_t* post_off, const int32_t* post_idx,
                          const float* post_w);
/* the fused sparse E-step on a diagonal model: scores on gselect [rows][n], the fp32 softmax of xv_ubm_post (min_post = 0), the
 * accumulation.  loglikes [rows][n] may be NULL; logsum [rows] comes back. */
xv_status xv_dgmm_acc_add_gselect(xv_dgmm_acc* a, const xv_ubm* diag, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  float* loglikes, float* logsum);
/* a caller's dense posteriors post [rows][G] through the matrix-core accumulation kernel and the reduction alone */
xv_status xv_dgmm_acc_add_dense_post(xv_dgmm_acc* a, const float* feats, int32_t rows, const float* post);
/* the fused dense E-step: every frame against every Gaussian.  logsum [rows] (may be NULL) comes back. */
xv_status xv_dgmm_acc_add_dense(xv_dgmm_acc* a, const xv_ubm* diag, const float* feats, int32_t rows, float* logsum);
/* downloads occ [G], mean [G][D] and var [G][D] (the sums of p x x); any of them may be NULL */
xv_status xv_dgmm_acc_get(const xv_dgmm_acc* a, double* occ, double* mean, double* var);
/* host only (fp64): the M-step of gmm-global-est on host arrays, then Split(mix_up, perturb_factor) keyed by seed when mix_up is above
 * the number of Gaussians that survive.  weights, means_invvars [.][D], inv_vars [.][D] and gconsts have room for max(num_gauss,
 * mix_up) Gaussians; the first num_gauss are read, the first *num_gauss_out are written.  removed [num_gauss]: the first entries are
 * the indices taken out, *num_removed (may be NULL with removed) how many.  floored2 = {variances floored, Gaussians they belong to};
 * objf3 = {the objective before, after, the sum of occ}; split_of [max(0, mix_up)]: for every Gaussian the split added, the index it
 * was copied from.  removed, floored2, objf3 and split_of may be NULL. */
xv_status xv_dgmm_est(int32_t num_gauss, int32_t dim, const char* acc_flags, const double* occ, const double* mean, const double* var,
                      const char* update_flags, double min_gaussian_weight, double min_gaussian_occupancy, double min_variance,
                      int32_t remove_low_count_gaussians, int32_t mix_up, double perturb_factor, uint64_t seed, float* weights,
                      float* means_invvars, float* inv_vars, float* gconsts, int32_t* num_gauss_out, int32_t* removed, int32_t* num_removed,
                      int32_t* floored2, double* objf3, int32_t* split_of);
/* the kernels' times in ms, the best of reps runs after one that warms up: ms7 = {sort, selected scores, softmax, sparse accumulation
 * (work items and reduction included)} of one fused sparse call when gselect is not NULL, then {dense log-sum, dense accumulation,
 * reduction} of one fused dense call when dense is not 0.  Every run adds to the accumulators. */
xv_status xv_dgmm_acc_kernel_time(xv_dgmm_acc* a, const xv_ubm* diag, const float* feats, int32_t rows, const int32_t* gselect, int32_t n,
                                  int32_t dense, int32_t reps, float* ms7);

/* ---- i-vector extraction (ivector-extract, sid/extract_ivectors.sh:69), without a model context.  Semantics: csrc/ivex.h.
 * Everything on the device is fp64 on fp32 inputs with summation orders that depend on the utterance and the model alone: an
 * utterance's results are the same bits alone, in any batch, at any position in it.  Limits: i-vector dimension <= 1024, feature
 * dimension <= 96.  A model with i-vector-dependent weights (a <w> matrix with rows) is refused by name. */
typedef struct xv_ivex xv_ivex;
/* Host arrays: w_vec [G], M [G][D][S], sigma_inv [G][D (D + 1) / 2] (packed lower triangles).  The derived variables SigmaInvM and
 * U are computed on the device here, once; the workspaces of a launch group are allocated here. */
xv_status xv_ivex_create(int device, int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, const double* w_vec, const double* M,
                         const double* sigma_inv, double prior_offset, xv_ivex** out);
/* the same from a final.ie, binary or text: "file", "-", "cmd |" */
xv_status xv_ivex_load(int device, const char* rxfilename, xv_ivex** out);
void xv_ivex_destroy(xv_ivex* m);
xv_status xv_ivex_info(const xv_ivex* m, int32_t* num_gauss, int32_t* feat_dim, int32_t* ivector_dim);
/* downloads sigma_inv_m [G D][S] and U [G][S (S + 1) / 2]; either may be NULL */
xv_status xv_ivex_derived(const xv_ivex* m, double* sigma_inv_m, double* U);
/* host buffers, blocking.  feats [row_off[n_utts]][D]; frame t has the pairs post_off[t] .. post_off[t + 1] (post_off has rows + 1
 * entries) of post_idx (Gaussian, in [0, G): anything else is XV_ERR_IO before anything is uploaded) and post_w.  ivectors
 * [n_utts][S] and status [n_utts] (0, or 1 for an utterance whose Q is not positive definite: its i-vector is then zero) are
 * always written; auxf_change [n_utts], gamma [n_utts][G], X [n_utts][G D], linear [n_utts][S] and quadratic
 * [n_utts][S (S + 1) / 2] (the packed lower triangle of Q) may each be NULL. */
xv_status xv_ivex_extract(xv_ivex* m, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off,
                          const int32_t* post_idx, const float* post_w, double acoustic_weight, double max_count, float* ivectors,
                          int32_t* status, double* auxf_change, double* gamma, double* X, double* linear, double* quadratic);
/* host only: a model file to host arrays and back (ivector-extractor-copy).  xv_ivex_read fills the three dimensions and whichever
 * of the arrays are not NULL: call it once for the shape and once for the data. */
xv_status xv_ivex_read(const char* rxfilename, int32_t* num_gauss, int32_t* feat_dim, int32_t* ivector_dim, double* w_vec, double* M,
                       double* sigma_inv, double* prior_offset);
xv_status xv_ivex_write(const char* wxfilename, int32_t binary, int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, const double* w_vec,
                        const double* M, const double* sigma_inv, double prior_offset);
/* the kernels' times in ms, the best of reps runs after one that warms up: ms5 = {statistics (sort included), quadratic GEMM, linear
 * GEMM (second pass included), solve, the derivation at model creation}; the first four summed over the call's launch groups */
xv_status xv_ivex_kernel_time(xv_ivex* m, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off,
                              const int32_t* post_idx, const float* post_w, int32_t reps, float* ms5);

/* ---- i-vector extractor training (ivector-extractor-init / -acc-stats / -sum-accs / -est, sid/train_ivector_extractor.sh:97-160).
 * Semantics: csrc/ivex_train.h.  The statistics are fp64 and a function of the model and the ordered sequence of accepted utterances
 * alone: how the utterances are split over calls changes no bit.  P = S (S + 1) / 2; packed arrays are lower triangles. */
typedef struct xv_ivex_acc xv_ivex_acc;
/* the accumulators on the model's device, at zero.  The model must outlive them. */
xv_status xv_ivex_acc_create(const xv_ivex* m, int32_t update_variances, int32_t compute_auxf, xv_ivex_acc** out);
void xv_ivex_acc_destroy(xv_ivex_acc* a);
/* the arguments of xv_ivex_extract.  status [n_utts] (may be NULL): 0, or 1 for an utterance whose Q is not positive definite: it
 * contributes to nothing. */
xv_status xv_ivex_acc_add(xv_ivex_acc* a, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off,
                          const int32_t* post_idx, const float* post_w, int32_t* status);
/* flushes what is pending and downloads: scalars3 = {num_ivectors, the objective, the weighted frame count}, gamma [G], Y [G][D][S],
 * R [G][P], Sg [G][D (D + 1) / 2] (written only with update_variances), ivector_sum [S], ivector_scatter [P].  Any may be NULL. */
xv_status xv_ivex_acc_get(xv_ivex_acc* a, double* scalars3, double* gamma, double* Y, double* R, double* Sg, double* ivector_sum,
                          double* ivector_scatter);
/* the pending utterances (fewer than 64) as the posterior kernel left them: m [count][S], scatter [count][P], logdet [count] (of
 * the posterior covariance) and auxf [count] (the utterance's part of the objective that needs the posterior).  Any may be NULL. */
xv_status xv_ivex_acc_pending(xv_ivex_acc* a, int32_t* count, double* m, double* scatter, double* logdet, double* auxf);
/* the kernels' times in ms of one xv_ivex_acc_add followed by a flush, the best of reps runs after one that warms up: ms3 =
 * {posterior kernel, R update, Y update}.  Every run adds the call's statistics to the accumulators. */
xv_status xv_ivex_acc_kernel_time(xv_ivex_acc* a, const float* feats, const int32_t* row_off, int32_t n_utts, const int32_t* post_off,
                                  const int32_t* post_idx, const float* post_w, int32_t reps, float* ms3);
/* the update kernel alone, on host arrays: C [c_rows][ldc] += A' B on rows < M and columns < N, A [64][M], B [64][N], of which the
 * first `slots` rows count.  c_rows >= M, ldc >= N: what lies outside [M][N] must come back untouched. */
xv_status xv_ivex_rank_update(int device, const double* A, const double* B, double* C, int32_t slots, int64_t M, int64_t N, int64_t c_rows,
                              int64_t ldc);
/* host only: ivector-extractor-init from a full-covariance UBM (weights [G], means_invcovars [G][D], inv_covars [G][D (D + 1) / 2]).
 * w_vec [G], M [G][D][S], sigma_inv [G][D (D + 1) / 2] and *prior_offset (100) are written.  The same seed gives the same bytes. */
xv_status xv_ivex_init(int32_t num_gauss, int32_t feat_dim, const float* weights, const float* means_invcovars, const float* inv_covars,
                       int32_t ivector_dim, uint64_t seed, double* w_vec, double* M, double* sigma_inv, double* prior_offset);
/* host only (fp64): the M-step of ivector-extractor-est.  Sg may be NULL without has_variances.  M, sigma_inv and *prior_offset are
 * updated in place.  counts6 = {Gaussians updated, skipped, eigenvalues of R floored, variances floored, Gaussians they belong to,
 * eigenvalues of the i-vector covariance floored}; impr3 = the objective improvements per frame of {projections, variances,
 * prior}; V [S][S]: the transform of the i-vectors the prior update applied.  The last three may be NULL. */
xv_status xv_ivex_est(int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, int32_t has_variances, const double* scalars3, const double* gamma,
                      const double* Y, const double* R, const double* Sg, const double* ivector_sum, const double* ivector_scatter,
                      double variance_floor_factor, double gaussian_min_count, int32_t diagonalize, int32_t num_threads, const double* w_vec, double* M,
                      double* sigma_inv, double* prior_offset, int32_t* counts6, double* impr3, double* V);
/* host only: the statistics file to host arrays and back.  xv_ivex_stats_read fills the shape and whichever arrays are not NULL. */
xv_status xv_ivex_stats_read(const char* rxfilename, int32_t* num_gauss, int32_t* feat_dim, int32_t* ivector_dim, int32_t* has_variances, double* scalars3,
                             double* gamma, double* Y, double* R, double* Sg, double* ivector_sum, double* ivector_scatter);
xv_status xv_ivex_stats_write(const char* wxfilename, int32_t binary, int32_t num_gauss, int32_t feat_dim, int32_t ivector_dim, int32_t has_variances,
                              const double* scalars3, const double* gamma, const double* Y, const double* R, const double* Sg, const double* ivector_sum,
                              const double* ivector_scatter);

/* ---- kernel-level entries of the frame-level and small kernels (unit tests; same conventions: device pointers from the caller
 * unless stated, an optional stream, XV_ERR_ARG with a reason for geometry a kernel cannot run, no engine or context) ---------- */
/* tdnn_first_kernel: the layer(s) that read the network input.  Chunk b holds rows [row_offsets[b], row_offsets[b + 1]) of feats
 * (row_offsets[0] may be > 0) and starts at device row dev_off[b]; device frame t of a chunk is its source frame
 * clamp(t - pad_left, 0, len - 1) for t < len + pad_left + pad_right; device rows outside every chunk read as zero.  The entry
 * builds the kernel's group table with the engine's own function, compacts both weight planes and launches rows
 * [row0, row0 + nrows).  Output pointers are indexed by absolute device row. */
typedef struct {
  const float* feats;            /* device fp32 [.. row_offsets[B]][dim] */
  const int32_t* row_offsets;    /* HOST [B + 1] */
  const int32_t* dev_off;        /* HOST [B], multiples of 16, chunks in increasing, non-overlapping order of device rows */
  int32_t B;
  int32_t rows;                  /* device rows, multiple of 64 */
  int32_t pad_left, pad_right;
  int32_t dim, noff;
  int32_t off[8];                /* time offsets in Append() order, each within +-15 */
  const void* w_hi; const void* w_lo;   /* 16-bit planes [n_pad][ldw] in the generic walk layout: segment j at column j * seg_pad */
  int32_t ldw, seg_pad;
  int32_t n_pad;                 /* multiple of 128 */
  int32_t epi_prec;              /* what the planes epilogue writes: XV_PREC_BF16X3 / XV_PREC_FP16X3 (hi + lo), XV_PREC_FP16X2 (fp16
                                  * plane only), XV_PREC_FP16X3E (fp16 plane + 4-bit residual); the products are three-pass */
  const float* bias; const float* scale; const float* offset;
  int32_t relu, bn;
  void* out_hi; void* out_lo; int32_t ldo;
  void* out_lo4; void* out_lo4_scale;
  void* gmax_out; const int8_t* out_range;   /* as in xv_gemm_desc */
  int32_t row0, nrows;           /* multiples of 64 */
  int32_t max_wgs;               /* > 0: at most this many workgroups per group of 512 columns (0: the launcher's rule) */
  void* hip_stream;
} xv_first_layer_desc;
xv_status xv_kernel_first_layer(const xv_first_layer_desc* d);
/* prep_input_kernel: fp32 rows -> 16-bit planes [rows][ld] (precision XV_PREC_BF16X3 .. XV_PREC_FP16X3; out_lo only for the split
 * ones), all tables on the device; zero_words (may be NULL): n_zero_words 32-bit words cleared by the same launch */
typedef struct {
  int32_t precision;
  const float* feats; const int32_t* src_off; const int32_t* dev_off; const int32_t* grp_utt;
  int32_t rows;                  /* multiple of 128 */
  int32_t dim, ld;               /* ld: multiple of 32, >= dim */
  void* out_hi; void* out_lo;
  int32_t pad_left, pad_right;
  void* zero_words; int32_t n_zero_words;
  void* hip_stream;
} xv_prep_input_desc;
xv_status xv_kernel_prep_input(const xv_prep_input_desc* d);
/* pool_finalise_kernel: per chunk b and column, the partials of groups [utt_grp0[b], utt_grp1[b]) -> mean | stddev as planes
 * [B][ld] (ld >= 2 dim) */
typedef struct {
  int32_t precision;             /* XV_PREC_BF16X3 .. XV_PREC_FP16X3 */
  const float* partial; int32_t ldp;   /* [groups][2][ldp] */
  const int32_t* utt_grp0; const int32_t* utt_grp1; const int32_t* utt_count;
  int32_t B, dim;
  float var_floor;
  void* out_hi; void* out_lo; int32_t ld;
  void* hip_stream;
} xv_pool_finalise_desc;
xv_status xv_kernel_pool_finalise(const xv_pool_finalise_desc* d);
/* frame_output kernels: out[o][0 .. dim) = (log-softmax of) row out_row[o] (o when out_row is NULL) of src [..][ld]; src16: the
 * logits as fp16 instead (log_softmax only, dim <= 16384) */
typedef struct {
  const float* src; const void* src16; int32_t ld;
  const int32_t* out_row; int32_t n_out;
  int32_t dim, log_softmax;
  float* out; int32_t out_ld;
  void* hip_stream;
} xv_frame_output_desc;
xv_status xv_kernel_frame_output(const xv_frame_output_desc* d);
/* bucket_sort kernels, HOST arrays in and out (the entry owns the device buffers): the stable counting sort by key that the UBM,
 * GMM and i-vector statistics start with.  keys [pairs], each in [0, num_keys); seg_off [num_segments + 1] rises from 0 to pairs,
 * 1 <= num_segments <= 64.  Inside every segment [seg_off[s], seg_off[s + 1]) the pairs are bucketed by key, ascending pair
 * index inside a bucket: sorted_out [pairs] holds the pair indices, bucket_start_out [num_segments][num_keys + 1] the absolute
 * position of every bucket (row s runs from seg_off[s] to seg_off[s + 1]).  XV_ERR_ARG, before anything is launched, for a key
 * out of range and for a segment table or sizes the launcher refuses. */
xv_status xv_bucket_sort(int32_t device, const int32_t* keys, int64_t pairs, const int32_t* seg_off, int32_t num_segments,
                         int32_t num_keys, int32_t* bucket_start_out, int32_t* sorted_out);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_HIP_H_ */
