"""The feature front-end without a model context: MFCC, energy VAD, wave files, reverberation, compression, CMVN, deltas."""
import ctypes
import os
from ctypes import byref

import numpy as np

from ._abi import XV_ERR_ARG, MfccOptions, ReverbOptions, VadOptions, XvError, _check, lib
from ._marshal import _f32, _f64, _i32, _pack_matrices, _ptr, _ptr_or_null, _ragged, _require, _split

WINDOW_TYPES = {"povey": 0, "hamming": 1, "hanning": 2, "rectangular": 3, "blackman": 4}
_MFCC_ALIASES = {"frame_length": "frame_length_ms", "frame_shift": "frame_shift_ms"}


def _options(struct, default_fn, opts, what):
    """the library's defaults of an options struct with keyword overrides"""
    o = struct()
    getattr(lib(), default_fn)(byref(o))
    names = {n for n, _ in struct._fields_}
    for k, v in opts.items():
        _require(k in names, "unknown %s option %r" % (what, k))
        setattr(o, k, v)
    return o


def mfcc_options(**opts):
    """Kaldi's compute-mfcc-feats defaults (xv_mfcc_options_default) with overrides named like the command-line options
    (underscores for dashes): sample_frequency, frame_length, frame_shift, dither, preemphasis_coefficient, remove_dc_offset,
    window_type (a name), blackman_coeff, round_to_power_of_two, snip_edges, num_mel_bins, low_freq, high_freq, num_ceps,
    cepstral_lifter, use_energy, raw_energy, energy_floor."""
    opts = {_MFCC_ALIASES.get(k, k): v for k, v in opts.items()}
    w = opts.get("window_type")
    if isinstance(w, str):
        _require(w in WINDOW_TYPES, "Invalid window type %s" % w)
        opts["window_type"] = WINDOW_TYPES[w]
    return _options(MfccOptions, "xv_mfcc_options_default", opts, "MFCC")


def mfcc_num_frames(n_samples, **opts):
    """Frames Kaldi extracts from n_samples samples under these options (host only)."""
    o = opts["options"] if "options" in opts else mfcc_options(**opts)
    n = lib().xv_mfcc_num_frames(byref(o), int(n_samples))
    if n < 0:
        raise XvError(XV_ERR_ARG, lib().xv_last_error().decode(errors="replace"))
    return int(n)


def utt_seed(key):
    """The 64-bit hash of an utterance key that keys the dither generator (xv_mfcc_utt_seed)."""
    return int(lib().xv_mfcc_utt_seed(key.encode()))


def _all_int16(waves):
    return len(waves) > 0 and all(np.asarray(w).dtype == np.int16 for w in waves)


def mfcc(waves, keys=None, device=0, **opts):
    """MFCCs of a list of waveforms on the device (compute-mfcc-feats): waves are 1-d arrays in Kaldi's unscaled range, all
    int16 (converted on the device) or anything else (taken as float32).  keys name the utterances for the dither generator
    (default "0", "1", ...; unused with dither=0).  Returns a list of float32 [frames, num_ceps] arrays."""
    L = lib()
    o = opts.pop("options") if "options" in opts else mfcc_options(**opts)
    i16 = _all_int16(waves)
    samples, off = _ragged(waves, np.int16 if i16 else np.float32)
    n = len(waves)
    if keys is None:
        keys = [str(i) for i in range(n)]
    seeds = np.array([utt_seed(k) for k in keys], dtype=np.uint64)
    frames = [mfcc_num_frames(off[u + 1] - off[u], options=o) for u in range(n)]
    out = np.empty((max(1, sum(frames)), o.num_ceps), dtype=np.float32)
    row_off = np.zeros(n + 1, dtype=np.int32)
    fn = L.xv_mfcc_compute_i16 if i16 else L.xv_mfcc_compute
    _check(fn(device, byref(o), samples.ctypes.data, off.ctypes.data, n, seeds.ctypes.data if n else None, out.ctypes.data,
              row_off.ctypes.data))
    assert list(np.diff(row_off)) == frames
    return _split(out, row_off)


def vad(feats, device=0, vad_energy_threshold=5.0, vad_energy_mean_scale=0.5, vad_proportion_threshold=0.6, vad_frames_context=0):
    """Kaldi's energy VAD (compute-vad) on the device for a list of float32 [frames, dim] feature matrices (column 0 = log
    energy).  Returns a list of float32 [frames] arrays of 1.0 / 0.0."""
    fs = [_f32(f) for f in feats]
    dim = fs[0].shape[1] if fs else 1
    _require(all(f.ndim == 2 and f.shape[1] == dim for f in fs), "vad: every feature matrix must be [frames, %d]" % dim)
    off = np.zeros(len(fs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([f.shape[0] for f in fs])
    packed = np.concatenate(fs, axis=0) if fs else np.zeros((0, dim), np.float32)
    out = np.empty(max(1, int(off[-1])), dtype=np.float32)
    o = VadOptions(vad_energy_threshold, vad_energy_mean_scale, vad_proportion_threshold, vad_frames_context)
    _check(lib().xv_vad_energy(device, byref(o), _ptr_or_null(packed), off.ctypes.data, len(fs), dim, out.ctypes.data))
    return _split(out, off)


def read_wave(rxfilename, channel=-1):
    """Reads a 16-bit PCM RIFF/WAVE from a file or a "cmd |" pipe the way compute-mfcc-feats does (xv_wave_read; host only).
    Returns (rate, int16 array of the chosen channel)."""
    L = lib()
    rate, n = ctypes.c_int32(0), ctypes.c_int64(0)
    p = ctypes.POINTER(ctypes.c_int16)()
    _check(L.xv_wave_read(os.fsencode(rxfilename), channel, byref(rate), byref(p), byref(n)))
    try:
        x = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int16)
    finally:
        L.xv_wave_free(p)
    return rate.value, x


def write_wave(wxfilename, samples, rate):
    """Writes a 1-d array as one channel of 16-bit PCM RIFF/WAVE to a file, "-" or "| cmd" (xv_wave_write; host only): values
    are truncated toward zero and saturated to the 16-bit range.  Returns how many were saturated."""
    x = _f32(samples).reshape(-1)
    clipped = ctypes.c_int64(0)
    _check(lib().xv_wave_write(os.fsencode(wxfilename), int(rate), _ptr_or_null(x), x.size, byref(clipped)))
    return clipped.value


def _recognize(fn_name, text):
    """None, or the dict of the "name=value" lines a recogniser of the library describes a pipeline with"""
    found = ctypes.c_int32(0)
    buf = ctypes.create_string_buffer(1 << 16)
    _check(getattr(lib(), fn_name)(text.encode(), byref(found), buf, len(buf)))
    if not found.value:
        return None
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def recognize_cmvn_pipeline(rspecifier):
    """None, or the fields of the per-speaker feature pipeline nnet3-compute runs on the device instead of as commands
    (xv_recognize_cmvn_pipeline, csrc/fuse_pipe.h; host only): {"stats", "stats-is-table", "feats", "vad", "utt2spk", "norm-means",
    "norm-vars"}, all strings ("vad" / "utt2spk" empty when the string has none)."""
    return _recognize("xv_recognize_cmvn_pipeline", rspecifier)


def recognize_wav_pipeline(rxfilename):
    """None, or the fields of the wav-reverberate line compute-mfcc-feats would take over instead of running it
    (xv_recognize_wav_pipeline; host only): a dict of the "name=value" lines, e.g. "source", "impulse-response", "duration",
    "additive[0].rx", "additive[1].source"."""
    return _recognize("xv_recognize_wav_pipeline", rxfilename)


def reverb_options(**opts):
    """wav-reverberate's defaults (xv_reverb_options_default) with overrides named like the command-line options (underscores
    for dashes): shift_output, normalize_output, duration, volume, input_wave_channel, rir_channel, noise_channel."""
    return _options(ReverbOptions, "xv_reverb_options_default", opts, "wav-reverberate")


def reverb_output_length(n_samples, rir_len=0, rate=8000.0, **opts):
    """Samples wav-reverberate writes for an input of n_samples and a RIR of rir_len taps (0: none); host only."""
    o = opts["options"] if "options" in opts else reverb_options(**opts)
    return int(lib().xv_reverb_output_length(byref(o), float(rate), int(n_samples), int(rir_len)))


def reverberate(waves, rirs=None, additive=None, rate=8000.0, device=0, return_int16=False, kernel_time_reps=0, **opts):
    """wav-reverberate on the device for a list of waveforms (1-d arrays in the 16-bit range, all int16 or taken as float32).
    rirs: None, or one entry per waveform: None, an array (the impulse response as read from its file, not scaled), or an int
    index into `rir_list=` given among the options (utterances naming the same index share its spectra).  additive: None, or
    per waveform a list of (noise array, snr dB, start seconds).  Options are named like the command line's (shift_output,
    normalize_output, duration, volume).  Returns a list of float32 arrays (the signal before quantisation); with
    return_int16 a list of (float32, int16, clipped count).  kernel_time_reps > 0: returns the kernels' time in ms instead
    (xv_reverb_kernel_time)."""
    L = lib()
    rir_list = list(opts.pop("rir_list", []))
    o = opts.pop("options") if "options" in opts else reverb_options(**opts)
    i16 = _all_int16(waves)
    samples, off = _ragged(waves, np.int16 if i16 else np.float32)
    n = len(waves)
    utt_rir = np.full(max(1, n), -1, dtype=np.int32)
    if rirs is not None:
        _require(len(rirs) == n, "reverberate: one RIR entry per waveform")
        for u, r in enumerate(rirs):
            if r is None:
                continue
            if isinstance(r, (int, np.integer)):
                utt_rir[u] = int(r)
            else:
                rir_list.append(r)
                utt_rir[u] = len(rir_list) - 1
    rir_flat, rir_off = _ragged(rir_list, np.float32)
    noise_list, add_noise, add_snr, add_start = [], [], [], []
    add_off = np.zeros(n + 1, dtype=np.int32)
    if additive is not None:
        _require(len(additive) == n, "reverberate: one list of additive signals per waveform")
        for u, lst in enumerate(additive):
            for (x, snr, start) in (lst or []):
                noise_list.append(x)
                add_noise.append(len(noise_list) - 1)
                add_snr.append(snr)
                add_start.append(start)
            add_off[u + 1] = len(add_noise)
    noise_flat, noise_off = _ragged(noise_list, np.float32)
    add_noise = np.array(add_noise + [0], dtype=np.int32)
    add_snr = np.array(add_snr + [0], dtype=np.float32)
    add_start = np.array(add_start + [0], dtype=np.float32)
    lens = [reverb_output_length(off[u + 1] - off[u], rir_off[utt_rir[u] + 1] - rir_off[utt_rir[u]] if utt_rir[u] >= 0 else 0,
                                 rate, options=o) for u in range(n)]
    total = max(1, sum(max(0, x) for x in lens))
    common = (device, byref(o), float(rate), samples.ctypes.data, 1 if i16 else 0, off.ctypes.data, n,
              rir_flat.ctypes.data, rir_off.ctypes.data, len(rir_list), utt_rir.ctypes.data,
              noise_flat.ctypes.data, noise_off.ctypes.data, len(noise_list), add_off.ctypes.data if additive is not None else None,
              add_noise.ctypes.data, add_snr.ctypes.data, add_start.ctypes.data)
    if kernel_time_reps > 0:
        ms = ctypes.c_float(0)
        _check(L.xv_reverb_kernel_time(*common, int(kernel_time_reps), byref(ms)))
        return ms.value
    out = np.empty(total, dtype=np.float32)
    out16 = np.empty(total, dtype=np.int16) if return_int16 else None
    clipped = np.zeros(max(1, n), dtype=np.int64)
    out_off = np.zeros(n + 1, dtype=np.int64)
    _check(L.xv_wav_reverberate(*common, out_off.ctypes.data, out.ctypes.data, _ptr(out16), clipped.ctypes.data))
    assert list(np.diff(out_off)) == [max(0, x) for x in lens]
    if return_int16:
        return [(a, b, int(clipped[u])) for u, (a, b) in enumerate(zip(_split(out, out_off), _split(out16, out_off)))]
    return _split(out, out_off)


def compressed_size(rows, cols, method=1):
    """(bytes of the object that follows the token, "CM" / "CM2" / "CM3") of a rows x cols matrix: host only."""
    n, fmt = ctypes.c_size_t(0), ctypes.c_char_p()
    _check(lib().xv_compressed_size(rows, cols, method, byref(n), byref(fmt)))
    return int(n.value), fmt.value.decode()


def compress(mats, method=1, device=0, return_flags=False, kernel_time_reps=0):
    """Kaldi's compressed matrices (copy-feats --compress=true) of a list of float32 matrices that share their column count, on
    the device.  Returns a list of `bytes`, each what follows the "CM " / "CM2 " / "CM3 " token (compressed_size names the
    token); with return_flags also the list of flags that mark the matrices holding a value that is not finite, whose bytes
    mean nothing.  kernel_time_reps > 0: returns the kernels' time in ms instead (xv_compress_kernel_time)."""
    L = lib()
    packed, off, cols = _pack_matrices(mats, "compress")
    n = len(off) - 1
    common = [device, _ptr_or_null(packed), off.ctypes.data, n, cols, method]
    if kernel_time_reps > 0:
        ms = ctypes.c_float(0)
        _check(L.xv_compress_kernel_time(*common, int(kernel_time_reps), byref(ms)))
        return ms.value
    total = sum(compressed_size(int(off[u + 1] - off[u]), cols, method)[0] for u in range(n))
    out = np.zeros(max(1, total), dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int64)
    flags = np.zeros(max(1, n), dtype=np.int32)
    _check(L.xv_compress_matrices(*common, out.ctypes.data, out_off.ctypes.data, flags.ctypes.data))
    assert int(out_off[n]) == total
    objs = [out[out_off[u]:out_off[u + 1]].tobytes() for u in range(n)]
    return (objs, [bool(f) for f in flags[:n]]) if return_flags else objs


def cmvn_sliding(mats, cmn_window=600, min_cmn_window=100, center=False, device=0):
    """apply-cmvn-sliding --norm-vars=false on the device, without a model: a list of float32 [frames, dim] matrices in, the
    same shapes out (the kernels of Context.frontend with every frame kept)."""
    packed, off, cols = _pack_matrices(mats, "cmvn_sliding")
    out = np.empty_like(packed)
    _check(lib().xv_cmvn_sliding(device, _ptr_or_null(packed), off.ctypes.data, len(off) - 1, max(cols, 1), cmn_window,
                                 min_cmn_window, 1 if center else 0, _ptr_or_null(out)))
    return _split(out, off)


def cmvn_stats(feats_list, device=0, kernel_time_reps=0):
    """Kaldi's CMVN statistics (compute-cmvn-stats) of a list of float32 [frames, cols] matrices that share their column count, summed
    on the device in fp64: a float64 array [n][2][cols + 1] - row 0 the column sums and the frame count, row 1 the sums of squares and
    0.  A matrix's statistics do not depend on the batch it is in.  kernel_time_reps > 0: (stats_ms, apply_ms) of xv_cmvn_kernel_time."""
    L = lib()
    packed, off, cols = _pack_matrices(feats_list, "cmvn_stats")
    n = len(off) - 1
    _require(cols >= 1, "cmvn_stats: no matrix with rows and columns")
    if kernel_time_reps > 0:
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        _check(L.xv_cmvn_kernel_time(device, packed.ctypes.data, off.ctypes.data, n, cols, int(kernel_time_reps), byref(a), byref(b)))
        return a.value, b.value
    stats = np.zeros((n, 2, cols + 1), dtype=np.float64)
    _check(L.xv_cmvn_stats(device, _ptr_or_null(packed), off.ctypes.data, n, cols, stats.ctypes.data, None))
    return stats


def cmvn_norm(stats, norm_means=True, norm_vars=False, reverse=False, skip_dims=(), return_floored=False):
    """One [2][cols + 1] statistics matrix -> float32 [2][cols]: row 0 the offset, row 1 the scale of out = x * scale + offset
    (xv_cmvn_norm: fp64 arithmetic, host only)."""
    st = _f64(stats)
    _require(st.ndim == 2 and st.shape[0] == 2 and st.shape[1] >= 2, "cmvn_norm: the statistics are a [2][cols + 1] matrix")
    cols = st.shape[1] - 1
    skip = _i32(list(skip_dims))
    norm = np.zeros((2, cols), dtype=np.float32)
    floored = ctypes.c_int32(0)
    _check(lib().xv_cmvn_norm(st.ctypes.data, cols, int(bool(norm_means)), int(bool(norm_vars)), int(bool(reverse)),
                              _ptr_or_null(skip), int(skip.size), norm.ctypes.data, byref(floored)))
    return (norm, int(floored.value)) if return_floored else norm


def apply_cmvn(feats_list, norms, utt_norm, device=0):
    """out = x * scale + offset on the device (apply-cmvn): matrix u of feats_list takes norms[utt_norm[u]] ([2][cols] each, as cmvn_norm
    returns them).  fp32, the product and the sum each rounded on their own.  Returns the list of normalised matrices."""
    packed, off, cols = _pack_matrices(feats_list, "apply_cmvn")
    n = len(off) - 1
    nm, un = _f32(norms), _i32(utt_norm)
    _require(un.shape == (n,) and nm.ndim == 3 and nm.shape[1:] == (2, max(cols, 1)) and not (n and (un.min() < 0 or un.max() >= nm.shape[0])),
             "apply_cmvn: norms are [n_norms][2][cols] and utt_norm names one of them per matrix")
    out = np.empty_like(packed)
    _check(lib().xv_cmvn_apply(device, _ptr_or_null(packed), off.ctypes.data, n, max(cols, 1), nm.ctypes.data, un.ctypes.data,
                               _ptr_or_null(out)))
    return _split(out, off)


def apply_cmvn_select(feats_list, norms, utt_norm, sel_row, sel_utt, device=0):
    """The same map behind a row selection, as one launch (xv_cmvn_apply_select): row i of the result is row sel_row[i] of the
    packed matrices (an absolute row, inside matrix sel_utt[i]) times the scale plus the offset of norms[utt_norm[sel_utt[i]]].  A
    matrix without a selected row may have utt_norm -1.  Returns one float32 [len(sel_row), cols] matrix."""
    packed, off, cols = _pack_matrices(feats_list, "apply_cmvn_select")
    n = len(off) - 1
    cols = max(cols, 1)
    nm, un, sr, su = _f32(norms), _i32(utt_norm), _i32(sel_row), _i32(sel_utt)
    _require(un.shape == (n,) and nm.ndim == 3 and nm.shape[1:] == (2, cols) and sr.ndim == 1 and sr.shape == su.shape,
             "apply_cmvn_select: norms are [n_norms][2][cols], utt_norm has one entry per matrix, sel_row and sel_utt one per kept row")
    out = np.empty((sr.size, cols), dtype=np.float32)
    _check(lib().xv_cmvn_apply_select(device, _ptr_or_null(packed), off.ctypes.data, n, cols, _ptr_or_null(nm), int(nm.shape[0]),
                                      _ptr_or_null(un), _ptr_or_null(sr), _ptr_or_null(su), int(sr.size), _ptr_or_null(out)))
    return out


def add_deltas(feats_list, order=2, window=2, truncate=0, device=0):
    """add-deltas on the device: a list of float32 [frames, cols] matrices that share their column count in, the matrices of
    (order + 1) * (truncate or cols) columns out.  fp32, every product and every sum rounded on its own (csrc/ubm.h)."""
    packed, off, cols = _pack_matrices(feats_list, "add_deltas")
    _require(cols >= 1, "add_deltas: no matrix with rows and columns")
    oc = (order + 1) * (truncate if truncate > 0 else cols)
    out = np.zeros((packed.shape[0], max(oc, 1)), dtype=np.float32)
    _check(lib().xv_add_deltas(device, packed.ctypes.data, off.ctypes.data, len(off) - 1, cols, order, window, truncate, out.ctypes.data, None))
    return _split(out, off)
