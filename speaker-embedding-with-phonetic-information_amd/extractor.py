"""The extractor: a model on the host, its context on one device, calibration and its shared file, the chunk plan."""
import ctypes
import os
import sys
from ctypes import byref

import numpy as np

from ._abi import PREC_DEFAULT, PRECISION_NAMES, PRECISIONS, XV_OK, Calibration, ModelInfo, _check, _Handle, lib
from ._marshal import _f32, _i32, _ptr


class Model(_Handle):
    """Parsed nnet3 model lowered to a TDNN program (host only; works without a GPU)."""
    _destroy = "xv_model_free"

    def __init__(self, raw=None, rxfilename=None, nnet_config=None, output_node=None):
        L = lib()
        self._h = ctypes.c_void_p()
        cfg = nnet_config.encode() if nnet_config else None
        node = output_node.encode() if output_node else None
        if raw is not None:
            buf = ctypes.create_string_buffer(bytes(raw), len(raw))
            _check(L.xv_model_load(buf, len(raw), cfg, node, byref(self._h)))
        else:
            _check(L.xv_model_load_rxfilename(rxfilename.encode(), cfg, node, byref(self._h)))

    @property
    def info(self):
        mi = ModelInfo()
        _check(lib().xv_model_info(self._h, byref(mi)))
        return mi

    def macs(self, frames):
        return lib().xv_model_macs(self._h, int(frames))

    def describe(self):
        n = lib().xv_model_describe(self._h, None, 0)
        buf = ctypes.create_string_buffer(n)
        lib().xv_model_describe(self._h, buf, n)
        return buf.value.decode()

    def pack(self, precision=PREC_DEFAULT):
        n = ctypes.c_size_t(0)
        _check(lib().xv_model_pack(self._h, precision, None, byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        _check(lib().xv_model_pack(self._h, precision, buf, byref(n)))
        return buf.raw[:n.value]


class Context(_Handle):
    """Weights resident on one MI355X + workspaces.  Raises XvError(XV_ERR_DEVICE) without a gfx950 GPU."""
    _destroy = "xv_ctx_free"

    def __init__(self, model=None, blob=None, device=0, precision=PREC_DEFAULT, device_blob=None, _handle=None):
        """device_blob = (device pointer as int, nbytes): the packed image already in this GPU's memory (e.g. the
        buffer a RCCL broadcast filled); the weights then never visit the host."""
        L = lib()
        self._h = ctypes.c_void_p(_handle)
        if _handle is not None:
            pass
        elif device_blob is not None:
            _check(L.xv_ctx_create_from_device_blob(ctypes.c_void_p(int(device_blob[0])), int(device_blob[1]), device, byref(self._h)))
        elif blob is not None:
            self._blob = ctypes.create_string_buffer(bytes(blob), len(blob))
            _check(L.xv_ctx_create_from_blob(self._blob, len(blob), device, byref(self._h)))
        else:
            _check(L.xv_ctx_create(model._h, device, precision, byref(self._h)))
        mi = ModelInfo()
        p, d = ctypes.c_int32(), ctypes.c_int32()
        _check(L.xv_ctx_info(self._h, byref(mi), byref(p), byref(d)))
        self.info, self.precision, self.device = mi, p.value, d.value

    def forward_batch(self, feats, row_offsets):
        """feats: float32 numpy [rows, input_dim]; row_offsets: int32 [B+1] -> numpy [B, output_dim]."""
        feats, offs = _f32(feats), _i32(row_offsets)
        B = len(offs) - 1
        # segment-level models: one row per chunk; frame-level models: one row per input frame
        n_out = B if self.info.output_is_segment else int(offs[-1] - offs[0])
        out = np.empty((n_out, self.info.output_dim), dtype=np.float32)
        _check(lib().xv_forward_batch(self._h, feats.ctypes.data, offs.ctypes.data, B, out.ctypes.data))
        return out

    def forward_batch_device(self, feats_ptr, row_offsets, out_ptr, out_ld, stream=None):
        """Device pointers (ints); asynchronous on `stream` (a hipStream_t as int, None = context stream)."""
        offs = _i32(row_offsets)
        _check(lib().xv_forward_batch_device(self._h, feats_ptr, offs.ctypes.data, len(offs) - 1, out_ptr, out_ld, stream))

    def synchronize(self):
        _check(lib().xv_ctx_synchronize(self._h))

    def set_profiling(self, on):
        _check(lib().xv_ctx_set_profiling(self._h, 1 if on else 0))

    def profile_report(self):
        """[(label, launches, total_ms)] of everything recorded since the last call."""
        buf = ctypes.create_string_buffer(1 << 18)   # one call: reading the report resets it
        lib().xv_ctx_profile_report(self._h, buf, len(buf))
        rows = []
        for line in buf.value.decode().splitlines():
            label, calls, ms = line.split("\t")
            rows.append((label, int(calls), float(ms)))
        return rows

    def frontend(self, raw, raw_offsets, vad=None, cmn_window=300, center=True):
        """apply-cmvn-sliding (norm-vars=false) + select-voiced-frames on the device.  Returns (feats, offsets)."""
        raw, offs = _f32(raw), _i32(raw_offsets)
        n = len(offs) - 1
        out = np.empty_like(raw)
        out_off = np.zeros(n + 1, dtype=np.int32)
        v = None if vad is None else _f32(vad)
        _check(lib().xv_frontend_cmvn_select(self._h, raw.ctypes.data, offs.ctypes.data, n, _ptr(v), cmn_window, 1 if center else 0,
                                             out.ctypes.data, out_off.ctypes.data))
        return out[:out_off[-1]], out_off

    def extract_table(self, feature_rspecifier, vector_wspecifier, chunk_size=-1, min_chunk_size=100, pad_input=True,
                      batch_frames=0):
        """What one nnet3-xvector-compute process does, on this context.  Returns (done, failed)."""
        done, failed = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().xv_extract_table(self._h, feature_rspecifier.encode(), vector_wspecifier.encode(), chunk_size,
                                      min_chunk_size, 1 if pad_input else 0, batch_frames, byref(done), byref(failed)))
        return done.value, failed.value

    def calibrate(self, feats, row_offsets, tol=7.5e-5):
        """xv_ctx_calibrate on host chunks: picks the fastest arithmetic whose embeddings stay within tol of the three-pass
        ones ON THESE CHUNKS and switches the context to it.  Returns {"chosen": name, "checked", "err_mx", "err_mx2"}."""
        feats, offs = _f32(feats), _i32(row_offsets)
        c = Calibration()
        _check(lib().xv_ctx_calibrate(self._h, feats.ctypes.data, offs.ctypes.data, len(offs) - 1, tol, byref(c)))
        return c.as_dict()

    def calibrate_table(self, feature_rspecifier, chunk_size=-1, min_chunk_size=100, pad_input=True, max_utts=64, tol=7.5e-5):
        """The same on the first chunk of the first max_utts utterances of a feature table."""
        c = Calibration()
        _check(lib().xv_calibrate_table(self._h, feature_rspecifier.encode(), chunk_size, min_chunk_size, 1 if pad_input else 0,
                                        max_utts, tol, byref(c)))
        return c.as_dict()

    @property
    def fast_mode(self):
        """Name of the arithmetic the fast chunks run in right now (xv_ctx_fast_mode)."""
        p = ctypes.c_int32()
        _check(lib().xv_ctx_fast_mode(self._h, byref(p)))
        return PRECISION_NAMES.get(p.value, str(p.value))

    def set_fast_mode(self, name):
        _check(lib().xv_ctx_set_fast_mode(self._h, PRECISIONS[name]))

    @property
    def lite_mask(self):
        """Layers (bit = index) that run the 1.25-pass arithmetic inside the fp16mx2 context (xv_ctx_lite_layers)."""
        m = ctypes.c_uint64()
        _check(lib().xv_ctx_lite_layers(self._h, byref(m)))
        return int(m.value)

    def set_lite_mask(self, mask):
        _check(lib().xv_ctx_set_lite_layers(self._h, ctypes.c_uint64(int(mask))))

    def set_calibration(self, enable=True, tol=7.5e-5):
        """extract_table then calibrates on the head of its own table before the first batch."""
        _check(lib().xv_ctx_set_calibration(self._h, 1 if enable else 0, tol))

    @property
    def model_fingerprint(self):
        """Fingerprint of the packed model image this context runs (what a calibration file names)."""
        v = ctypes.c_uint64()
        _check(lib().xv_ctx_model_fingerprint(self._h, byref(v)))
        return int(v.value)

    def share_calibration(self, path, tol=7.5e-5, note=None):
        """The shared choice of a recipe (xv_ctx_share_calibration): applies the file's choice when it exists, else publishes this
        context's current choice atomically and adopts what the file then holds.  Returns "read" / "published" / "adopted"."""
        out = ctypes.c_int32(-1)
        _check(lib().xv_ctx_share_calibration(self._h, os.fsencode(path), ctypes.c_float(tol), note.encode() if note else None,
                                              byref(out)))
        return ("read", "published", "adopted")[out.value]

    def set_calibration_file(self, path):
        """extract_table applies / creates the shared calibration file before its first batch (None: off)."""
        _check(lib().xv_ctx_set_calibration_file(self._h, os.fsencode(path) if path else None))

    def extract_utterances(self, feats, row_offsets, chunk_size=-1, min_chunk_size=100, pad_input=True):
        feats, offs = _f32(feats), _i32(row_offsets)
        n = len(offs) - 1
        out = np.zeros((n, self.info.output_dim), dtype=np.float32)
        ok = np.zeros(n, dtype=np.int32)
        _check(lib().xv_extract_utterances(self._h, feats.ctypes.data, offs.ctypes.data, n, chunk_size, min_chunk_size,
                                           1 if pad_input else 0, out.ctypes.data, ok.ctypes.data))
        return out, ok.astype(bool)


class Watchdog:
    """Bounded wait for the start-up collective of a multi-rank job (the ONE broadcast of the packed weights, dist_extract.py /
    bench.py): a rank that never joins - died while loading, a link that is down - would otherwise leave the others inside
    the collective without a word until someone kills the job.  After `seconds` (XVEC_BCAST_TIMEOUT, default 120: the other
    ranks enter the broadcast while rank 0 still reads, lowers and packs the model - on a cold box that alone can take many seconds) the process
    prints what it was waiting for and EXITS with status 3; the launcher then tears the other ranks down.  A plain exit of a
    fresh-started process - nothing is re-executed (a process that has touched the GPU must never exec)."""

    def __init__(self, what, seconds=None):
        import threading
        if seconds is None:
            try:
                seconds = float(os.environ.get("XVEC_BCAST_TIMEOUT", "120"))
            except ValueError:
                seconds = 120.0
        self.what, self.seconds = what, seconds
        self._t = threading.Timer(seconds, self._fire)
        self._t.daemon = True
        self._t.start()

    def _fire(self):
        sys.stderr.write("ERROR (xvec_hip watchdog) rank %s: %s did not complete within %.0f s; exiting\n"
                         % (os.environ.get("RANK", "0"), self.what, self.seconds))
        sys.stderr.flush()
        os._exit(3)

    def cancel(self):
        self._t.cancel()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.cancel()
        return False


def create_broadcast(model, devices, precision=PREC_DEFAULT):
    """xv_ctx_create_broadcast: one process, one context per listed GPU; the packed weights are uploaded to the first
    device and broadcast with ONE ncclBroadcast (RCCL), each context is built from the image its device received."""
    n = len(devices)
    devs = (ctypes.c_int * n)(*devices)
    handles = (ctypes.c_void_p * n)()
    _check(lib().xv_ctx_create_broadcast(model._h, devs, n, precision, handles))
    return [Context(_handle=handles[i]) for i in range(n)]


def recognize_feature_pipeline(rspecifier):
    """The reference's feature pipeline as text (xv_recognize_feature_pipeline): {"feats", "vad", "cmn_window", "min_cmn_window",
    "center"} when the string is exactly `ark:apply-cmvn-sliding ... | select-voiced-frames ... |` with options the device
    front-end implements, else None."""
    found, w, mw, c = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    fb, vb = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    _check(lib().xv_recognize_feature_pipeline(rspecifier.encode(), byref(found), fb, 4096, vb, 4096, byref(w), byref(mw), byref(c)))
    if not found.value:
        return None
    return {"feats": fb.value.decode(), "vad": vb.value.decode(), "cmn_window": w.value, "min_cmn_window": mw.value, "center": bool(c.value)}


def _calibration_choice(model, prec, lite):
    return {"model": int(model.value), "precision": PRECISION_NAMES.get(prec.value, str(prec.value)), "lite_mask": int(lite.value)}


def calibration_file_read(path):
    """The shared choice a calibration file holds: {"model": fingerprint, "precision": name, "lite_mask": int}, or None when the
    file does not exist (xv_calibration_file_read; XvError when it cannot be parsed)."""
    found, prec = ctypes.c_int32(0), ctypes.c_int32(-1)
    model, lite = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().xv_calibration_file_read(os.fsencode(path), byref(found), byref(model), byref(prec), byref(lite)))
    return _calibration_choice(model, prec, lite) if found.value else None


def calibration_file_publish(path, model, precision, lite_mask=0, tol=7.5e-5, note=None):
    """Publishes a choice unless the file exists (atomic: the first of several concurrent publishers wins); returns
    (published, what the file holds afterwards)."""
    won, prec = ctypes.c_int32(0), ctypes.c_int32(-1)
    m, lite = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _check(lib().xv_calibration_file_publish(os.fsencode(path), ctypes.c_uint64(model), PRECISIONS[precision], ctypes.c_uint64(lite_mask),
                                             ctypes.c_float(tol), note.encode() if note else None, byref(won), byref(m), byref(prec),
                                             byref(lite)))
    return bool(won.value), _calibration_choice(m, prec, lite)


def plan_chunks(num_rows, chunk_size, min_chunk_size, pad_input, min_net_frames, cap=4096):
    """[(start, len, left_pad, right_pad)] or None when the utterance counts as failed (host logic, no GPU)."""
    arr = [(ctypes.c_int32 * cap)() for _ in range(4)]
    n = ctypes.c_int32(0)
    st = lib().xv_plan_chunks(num_rows, chunk_size, min_chunk_size, 1 if pad_input else 0, min_net_frames, cap, *arr, byref(n))
    if st != XV_OK:
        return None
    return [(arr[0][i], arr[1][i], arr[2][i], arr[3][i]) for i in range(n.value)]
