// The counter-based generator the device stages share (the MFCC dither of feat_kernels.hip, the random pruning of
// post_kernels.hip): 64 bits that are a function of (utterance seed, two 32-bit counters) and of nothing else, so that what a
// frame draws does not depend on the batch, the job split or the order of the work.  Device code only.
//   seed = FNV-1a (64 bit) of the utterance key (feat.h: UttSeed)
//   r    = mix64(mix64(seed ^ GOLDEN) + ((hi << 32) | lo) * GOLDEN)        mix64 = murmur3's 64-bit finaliser
//   u    = ((r >> 40) + 1) / 2^24 in (0, 1]: the top 24 bits, exact in fp32
// tests/dither_ref.py is the same in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xv {

__device__ inline uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}
__device__ inline uint64_t counter_bits(uint64_t seed, uint32_t hi, uint32_t lo) {
  const uint64_t ctr = ((uint64_t)hi << 32) | lo;
  return mix64(mix64(seed ^ 0x9e3779b97f4a7c15ULL) + ctr * 0x9e3779b97f4a7c15ULL);
}
// (0, 1], a multiple of 2^-24
__device__ inline float counter_unit_open0(uint64_t r) { return ((float)(uint32_t)(r >> 40) + 1.0f) * (1.0f / 16777216.0f); }

}  // namespace xv
