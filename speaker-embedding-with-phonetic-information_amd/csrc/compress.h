// Compressed feature matrices: what copy-feats --compress=true writes (steps/make_mfcc.sh:12, compress=true) and what the table
// readers of kio.cc and the device expansion (kernels.h CmExpandArgs) read back.  A restatement of Kaldi's CompressedMatrix of
// early 2018, in fp32 throughout; tests/compress_ref.py is the same in numpy, and the kernels (compress_kernels.hip) are compared
// with it byte for byte.
//
// Methods (--compression-method): 1 automatic ("CM" when rows > 8, else "CM2"), 2 "CM", 3 "CM2", 5 "CM3".  4, 6 and 7 (fixed
// ranges) are not built.
//
// Object = what follows the "CM " / "CM2 " / "CM3 " token:
//   float min, float range, int32 rows, int32 cols
//     min = the matrix minimum (a zero minimum is written as +0), max = the matrix maximum; max == min: max = min + (1 + |min|);
//     range = max - min
//   u16(x) = int(f * 65535 + 0.499), f = (x - min) / range clamped to [0, 1]
//   "CM":  uint16 percentiles[cols][4], then uint8 data[cols][rows] (column-major)
//     s = the sorted column, q = rows / 4 (integer); u0..u3 = u16 of s[0], s[q], s[3 q], s[rows - 1]  (3 q, not 3 rows / 4)
//     p0 = min(u0, 65532), p25 = min(max(u1, p0 + 1), 65533), p75 = min(max(u2, p25 + 1), 65534), p100 = max(u3, p75 + 1)
//     rows < 5: s[0], s[1], s[2], s[3] where they exist, the word before plus one where they do not
//     byte of v, with the DECODED percentiles P = min + range * 1.52590218966964e-05f * p (as the reader forms them):
//       v < P25:  clamp(int((v - P0) / (P25 - P0) * 64 + 0.5), 0, 64)
//       v < P75:  64 + clamp(int((v - P25) / (P75 - P25) * 128 + 0.5), 0, 128)
//       else:     192 + clamp(int((v - P75) / (P100 - P75) * 63 + 0.5), 0, 63)
//   "CM2": uint16 data[rows][cols] = int((v - min) / range * 65535 + 0.499);  "CM3": uint8, the same with 255
// A matrix without rows or columns is the 16-byte "CM" object of zeros.  A matrix that holds a NaN or an infinity, or whose range
// is not finite, is not compressed: the flag is set and the caller writes it as it is ("FM").
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace xv {

// false: a method that is not built.  *format: "CM", "CM2" or "CM3".
bool CompressedSize(int rows, int cols, int method, size_t* nbytes, const char** format);
// "compression method 4 ..." for the methods that are refused, "" for the others
std::string CompressionMethodError(int method);

// Compresses the n matrices feats[row_off[u] .. row_off[u + 1])[cols] on the device: object u goes to out_bytes + out_off[u],
// out_off[n + 1] is filled here (the objects follow each other without gaps, sizes as CompressedSize gives them).
// nonfinite[u] != 0: that object's bytes mean nothing.  Blocking.  device_ms: the kernels' time.
void CompressMatrices(int device, const float* feats, const int32_t* row_off, int n, int cols, int method, uint8_t* out_bytes,
                      int64_t* out_off, int32_t* nonfinite, float* device_ms = nullptr);

// apply-cmvn-sliding --norm-vars=false without a model context (the front-end's kernels, engine.h FrontEndRun): out has the
// shape of raw.
void CmvnSliding(int device, const float* raw, const int32_t* raw_off, int n, int cols, int cmn_window, int min_cmn_window,
                 bool center, float* out);

}  // namespace xv
