"""numpy restatement of logprob-to-post (csrc/post.h), written from its description and not from the library:

  per row, columns ascending:  a NaN is dropped;  p = exp(x[j]) rounded to float32;
    min_post <= 0: keep (j, p);   p >= min_post: keep (j, p);
    else with random_prune and p / min_post >= u: keep (j, min_post);   else drop
  u = the first uniform of tests/dither_ref.py for (utterance key, row within the utterance, column): a multiple of 2^-24 in (0, 1]

fp64=False decides in float32 as the tool does (p and p / min_post each rounded once); fp64=True decides on the float64 value of
exp, which is what the device test compares with after it has shown that no entry of its inputs is near a threshold."""
import numpy as np

import dither_ref

F = np.float32


def uniforms(key, rows, cols, row0=0):
    """[rows, cols] float64 u of rows row0 .. row0 + rows of utterance `key`"""
    return dither_ref.uniforms(key, row0 + rows, cols)[0][row0:]


def probabilities(x):
    """exp of the float32 log-probabilities in float64 (NaN stays NaN)"""
    with np.errstate(over="ignore"):
        return np.exp(np.asarray(x, F).astype(np.float64))


def thresholds(x, key, min_post, random_prune, row0=0):
    """per entry the threshold its p is compared with, in float64: min_post where p >= min_post decides, u * min_post for the entries
    below min_post with random pruning; NaN where nothing is compared (min_post <= 0, NaN input)"""
    x = np.asarray(x, F)
    mp = float(F(min_post))
    p = probabilities(x)
    t = np.full(x.shape, np.nan)
    if mp > 0:
        t[:] = mp
        if random_prune:
            u = uniforms(key, x.shape[0], x.shape[1], row0)
            t = np.where(p < mp, u * mp, t)
        t[np.isnan(p)] = np.nan
    return t


def near(x, key, min_post, random_prune, row0=0, ulps=4):
    """the entries whose float64 p lies within `ulps` float32 ulps of their threshold: where float32 and float64 may decide apart"""
    p = probabilities(x)
    t = thresholds(x, key, min_post, random_prune, row0)
    with np.errstate(invalid="ignore"):
        return np.abs(p - t) <= ulps * np.spacing(np.abs(t).astype(F)).astype(np.float64)


def logprob_to_post(x, key, min_post=0.01, random_prune=True, row0=0, fp64=False):
    """-> (per row (int32 columns, float32 weights), number of NaN inputs)"""
    x = np.asarray(x, F)
    rows, cols = x.shape
    mp32 = F(min_post)
    p64 = probabilities(x)
    with np.errstate(over="ignore"):
        p32 = p64.astype(F)
    nan = np.isnan(p64)
    if not mp32 > 0:
        keep, pruned = ~nan, np.zeros(x.shape, bool)
    else:
        p = p64 if fp64 else p32
        m = float(mp32) if fp64 else mp32
        with np.errstate(invalid="ignore"):
            full = p >= m
            pruned = np.zeros(x.shape, bool)
            if random_prune:
                u = uniforms(key, rows, cols, row0)
                q = p / m   # float32 / float32 is one correctly rounded division
                pruned = ~full & ~nan & (q >= (u if fp64 else u.astype(F)))
        keep = (full | pruned) & ~nan
    w = np.where(pruned, mp32, p32).astype(F)
    out = []
    for r in range(rows):
        j = np.nonzero(keep[r])[0].astype(np.int32)
        out.append((j, w[r, j]))
    return out, int(nan.sum())
