"""numpy restatement of the dither generator of the MFCC kernel, written from its description and not from the library:

  seed  = FNV-1a (64 bit) of the utterance key's bytes
  base  = mix64(seed ^ GOLDEN)                                  mix64 = murmur3's 64-bit finaliser
  r     = mix64(base + ((frame << 32) | sample) * GOLDEN)       all modulo 2^64; frame counts within the utterance
  u1    = ((r >> 40) + 1) / 2^24  in (0, 1]                     the top 24 bits
  u2    = ((r >> 8) & 0xffffff) / 2^24  in [0, 1)               the next 24 bits but 8
  draw  = sqrt(-2 ln u1) * cos(2 pi u2)                         Box-Muller

u1 and u2 are multiples of 2^-24 below 2, exact in fp32 as in fp64; the float64 evaluation of the last line is the truth
the kernel's fp32 logf / cosf is held to."""
import numpy as np

GOLDEN = np.uint64(0x9e3779b97f4a7c15)
_M = (1 << 64) - 1


def fnv1a(key):
    """64-bit FNV-1a of the key's UTF-8 bytes (plain Python integers)."""
    h = 0xcbf29ce484222325
    for b in key.encode():
        h = ((h ^ b) * 0x100000001b3) & _M
    return h


def mix64(x):
    """murmur3's fmix64 on a uint64 array (numpy's uint64 arithmetic wraps modulo 2^64)."""
    x = np.array(x, dtype=np.uint64, ndmin=1)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def uniforms(key, F, L):
    """([F, L] u1 in (0, 1], [F, L] u2 in [0, 1)) in float64."""
    base = mix64(np.uint64(fnv1a(key)) ^ GOLDEN)[0]
    ctr = (np.arange(F, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(L, dtype=np.uint64)[None, :]
    r = mix64(base + ctr * GOLDEN)
    u1 = ((r >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((r >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.float64) / 16777216.0
    return u1, u2


def draws(key, F, L):
    """[F, L] N(0, 1) draws in float64: row t is what frame t of utterance `key` adds (times --dither) to its L samples."""
    u1, u2 = uniforms(key, F, L)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
