"""The shapes of the i-vector GPU tests (tests/test_gpu_ivector.py, tests/test_gpu_ivector_train.py) and the inputs they are run on,
in one place: the GPU half runs them, the CPU half (tests/test_ivector_ref.py) checks on the restatement alone that every one of
them meets the preconditions the GPU tests assert.  Every threshold is read from the sources, so a list moves when a constant does.
No device, no library."""
import os
import re

import numpy as np

import ivector_ref as R

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "speaker-embedding-with-phonetic-information_amd", "csrc")


def _src(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _const(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


_HDR, _TRAIN_HDR, _HIP, _HOST = _src("ivex_kernels.h"), _src("ivex_train_kernels.h"), _src("ivex_kernels.hip"), _src("ivex.cc")
THREADS = _const(_HDR, "kIvexThreads")
RT = _const(_HDR, "kIvexRowTile")
CT = _const(_HDR, "kIvexColTile")
KC = _const(_HDR, "kIvexKChunk")
NB = _const(_HDR, "kIvexPanel")
MAX_S = _const(_HDR, "kIvexMaxS")
MAX_B = _const(_HDR, "kIvexMaxBatch")
MAX_D = _const(_HDR, "kIvexMaxDim")
POST_THREADS = _const(_TRAIN_HDR, "kIvexPosteriorThreads")
TRAIN_THREADS = _const(_TRAIN_HDR, "kIvexTrainThreads")
SLOTS = _const(_TRAIN_HDR, "kIvexTrainSlots")
SOLVE_RT = THREADS // int(re.search(r"constexpr int kSolveRowTile = kIvexThreads / (\d+);", _HIP).group(1))   # rows per pass of the block-column update
BATCH_FRAMES = 1 << int(re.search(r"constexpr int64_t kBatchFrames = 1 << (\d+);", _HOST).group(1))           # frames that close a launch group
WAVE = 64            # lanes of a gfx950 wavefront: the hardware's, not the project's
SOLVE_CARRY = 4      # entries of L's row a thread of the back substitution carries (cur[4], nxt[4])
assert SOLVE_CARRY * THREADS >= MAX_S
U53 = 2.0 ** -53


def eps_of(Q):
    """Higham's bound on the backward error of Cholesky, carried to the solution: cond_2(Q) 4 S (3 S + 1) 2^-53"""
    S = Q.shape[0]
    return np.linalg.cond(Q, 2) * 4 * S * (3 * S + 1) * U53


def m_scale_for(S):
    """The scale of a random model's M at i-vector dimension S.  Q - I is a sum of M_g' Sigma_g^-1 M_g, whose norm grows with S at a
    fixed scale: from S = 600 on the scale 0.3 gives eps_of(Q) above the 1e-6 the tests' inputs must stay under (1.9e-6 at 600, 7e-6
    at 1024).  0.3 sqrt(48 / S) keeps |Q - I| level.  Up to 2 NB + 3, the largest S of the tests before there was this rule, the
    scale is their 0.3 and the models are theirs."""
    return 0.3 if S <= 2 * NB + 3 else 0.3 * float(np.sqrt(48.0 / S))


# ------------------------------------------------------------------------------------------------------------------- the solve
# (G, D, S) of test_random_models_solve_within_the_bound.  The four first are the shapes the test has always had: S below, one
# above and two above the panel; (1, 2, 17) is the rank-poor case.
SOLVE_CASES = [(5, 7, 17), (6, 8, NB + 1), (6, 8, 2 * NB + 3), (1, 2, 17)]
# ivex_solve_kernel's loops over rows = S + 1, each one pass below its edge and two from it on:
#   NB + SOLVE_RT            the block-column update's row tile at k0 = NB: rows - NB > SOLVE_RT
#   THREADS, + 1, + 2        the loops that stride by the workgroup (unpack, auxf, outputs) at S = THREADS + 1; entry m = 1 of the back
#                            substitution's cur[] and nxt[] is first live (i = THREADS < j <= S - 1) at S = THREADS + 2
#   NB + THREADS             the triangular solve of the rows under the diagonal block at k0 = 0: NB + THREADS < rows
#   m THREADS + 1, + 2       entry m = 2 and m = 3 of cur[] and nxt[]
#   400, 600                 the recipes' dimensions
#   MAX_S - 1, MAX_S         the limit itself
SOLVE_EDGES = sorted({NB + SOLVE_RT - 1, NB + SOLVE_RT, THREADS, THREADS + 1, THREADS + 2, NB + THREADS - 1, NB + THREADS, 400, 600,
                      2 * THREADS + 1, 2 * THREADS + 2, 3 * THREADS + 1, 3 * THREADS + 2, MAX_S - 1, MAX_S})
SOLVE_CASES += [(5, 7, S) for S in SOLVE_EDGES if S <= MAX_S]


def solve_utts_count(S):
    return 3 if S < MAX_S - 1 else 2   # the reference costs O(S^3) per utterance


def solve_model(G, D, S):
    return R.random_model(7 * S + G, G, D, S, m_scale=m_scale_for(S))


def solve_utterances(G, D, S, n=3):
    """n utterances of 50, 67, 84 ... frames, up to three Gaussians a frame"""
    rng = np.random.default_rng(S)
    utts = []
    for u in range(n):
        T = 50 + 17 * u
        x = rng.normal(0.0, 2.0, (T, D)).astype(np.float32)
        post = []
        for t in range(T):
            idx = rng.permutation(G)[:min(G, 3)]
            w = rng.dirichlet(np.ones(len(idx))).astype(np.float32)
            post.append((idx.astype(np.int32), w))
        utts.append((x, post))
    return utts


# ------------------------------------------------------------------------------------------------------------------- integer models
def _shape_for(K):
    """(G, D) with G D = K and D the largest divisor of K that a model may have"""
    D = max(d for d in range(1, MAX_D + 1) if K % d == 0)
    return K // D, D


# (G, D, S, T, B): B around a row tile, S so that S and P fall on, below and above multiples of the column tile, G on and off
# multiples of 4, and G D one below, at and one above the linear term's K chunk and one above two chunks
CASES = [(37, 23, 40, 300, 1), (5, 60, 17, 64, RT + 1), (4, 1, 1, 3, RT - 1), (65, 24, 33, 500, 2 * RT + 1), (1, 23, 5, 20, RT),
         (3, 1, CT, 10, RT + 1), (4, 60, 5, 30, RT - 1), (1, 1, 1, 1, 1)]
CASES += [_shape_for(K) + (5, 40, b) for K, b in ((KC - 1, 1), (KC, RT), (KC + 1, RT + 1), (2 * KC + 1, 2))]
# the batch: the last row tile a wave of ivex_gemm carries begins at 3 RT + 1 utterances; MAX_B fills a launch group, one more opens
# a second group of one, 2 MAX_B + 2 makes three groups
BATCH_CASES = [(5, 6, 7, 60, b) for b in (3 * RT, 3 * RT + 1, MAX_B, MAX_B + 1, 2 * MAX_B + 2)]
# the feature dimension: lanes d + WAVE of ivex_stats are live from D = WAVE + 1, and ivex_derive holds Sigma^-1's triangle in LDS
DIM_CASES = [(3, d, 17, 30, 2) for d in (WAVE, WAVE + 1, MAX_D - 1, MAX_D)]
CASES += BATCH_CASES + DIM_CASES

# (G, D, S, T, B) whose terms are checked and whose solve is not: integer models are too ill-conditioned at this size for
# check_solve's precondition (SOLVE_CASES cover the solve).  P = MAX_S (MAX_S + 1) / 2 columns of the quadratic GEMM and the
# largest argument of ivex_derive's packed-index recovery.
LARGE_S_TERM_CASES = [(3, 2, THREADS + 1, 40, 3), (3, 2, MAX_S, 40, 2)]


def integer_seed(G, D, S):
    return 1000 * G + 10 * D + S


def integer_utterances(seed, B, T, G, D, **kw):
    """B utterances, every one with data and a length of its own"""
    return [R.integer_utterance(seed + 31 * u, max(1, T - 3 * u), G, D, **kw) for u in range(B)]


def case_utterances(G, D, S, T, B):
    return integer_utterances(G + D + S, B, T, G, D, empty_every=7)


def exact_preconditions(m, sim, U, x, post, gamma):
    """every absolute partial sum of l and Q stays below 2^53: float64 holds every one exactly, whatever the order"""
    abs_X = R.stats(np.abs(x), post, m["M"].shape[0])[1].reshape(-1)
    return bool((np.abs(sim).T @ abs_X).max() + abs(m["prior_offset"]) < 2.0 ** 53 and (gamma @ np.abs(U)).max() + 1.0 < 2.0 ** 53)


# a launch group closed by its frames (BATCH_FRAMES) and not by its utterances: the third utterance would take the first group past
# the limit, and the fourth is past it alone
FRAMES_SHAPE = (2, 1, 3)
_A = 11 * BATCH_FRAMES // 24   # about 30000
FRAMES_LENGTHS = [_A, _A - 300, _A + 200, BATCH_FRAMES + 500]
assert FRAMES_LENGTHS[0] + FRAMES_LENGTHS[1] <= BATCH_FRAMES < sum(FRAMES_LENGTHS[:3]) and FRAMES_LENGTHS[3] > BATCH_FRAMES


def long_integer_utterance(seed, T, G, D):
    """R.integer_utterance's value ranges with one Gaussian a frame, built without a loop over the frames"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, (T, D)).astype(np.float32)
    idx = rng.integers(0, G, T).astype(np.int32)
    w = (2.0 ** -rng.integers(0, 4, T)).astype(np.float32)
    return x, [(idx[t:t + 1], w[t:t + 1]) for t in range(T)]


def frames_utterances():
    G, D, _ = FRAMES_SHAPE
    return [long_integer_utterance(40 + u, T, G, D) for u, T in enumerate(FRAMES_LENGTHS)]


# ------------------------------------------------------------------------------------------------------------------- not positive definite
def not_pd_model(G, D, S, s0=0):
    """Sigma^-1 of Gaussian 0 has a negative diagonal, on purpose; s0 leading columns of every M_g are zero"""
    m = R.integer_model(5, G, D, S)
    m["sigma_inv"][0] = R.pack(-8.0 * np.eye(D))
    return R.zero_leading_columns(m, s0) if s0 else m


def not_pd_utterances(D):
    """a good one on Gaussian 1, the bad one on Gaussians 0 and 1 (drawn first), a good one"""
    rng = np.random.default_rng(1)
    good = lambda T: (rng.integers(-4, 5, (T, D)).astype(np.float32), [(np.array([1], np.int32), np.array([0.5], np.float32))] * T)
    bad = (rng.integers(-4, 5, (9, D)).astype(np.float32), [(np.array([0, 1], np.int32), np.array([1.0, 0.25], np.float32))] * 9)
    return [good(12), bad, good(5)]


LATE_S0, LATE_S = 2 * NB + 1, 3 * NB + 5   # no bad pivot in the two first panels


def first_bad_pivot(Q):
    """the index of the first pivot of an unpivoted Cholesky factorisation of Q that is not positive; len(Q) if there is none"""
    for k in range(1, len(Q) + 1):
        if np.linalg.eigvalsh(Q[:k, :k]).min() <= 0:
            return k - 1
    return len(Q)


# ------------------------------------------------------------------------------------------------------------------- training
# (G, D, S) of the posterior kernel's test.  The three first are the shapes it has always had.  k_first = tid & ~(WAVE - 1) is
# non-zero from the second wave on, S >= WAVE + 1, and S = WAVE + 2 is the first at which that wave has a product to add (row
# WAVE + 1 of Z, column WAVE); 2 WAVE and 2 WAVE + 1 add a third wave; 400 is the recipes'; MAX_S is where the packed-index
# recovery sees its largest argument and every thread of the workgroup owns a column.
POSTERIOR_CASES = [(5, 7, 6), (19, 33, 17), (8, 96, 33)]
POSTERIOR_CASES += [(5, 7, S) for S in sorted({WAVE - 1, WAVE, WAVE + 1, WAVE + 2, 2 * WAVE, 2 * WAVE + 1, 400, MAX_S - 1, MAX_S})]


def posterior_utts_count(S):
    return 4 if S <= 400 else 2


def posterior_model(G, D, S):
    return R.random_model(17 + S, G, D, S, m_scale=m_scale_for(S))


def random_utts(seed, n, G, D, lo=5, hi=40, scale=1.0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        frames = int(rng.integers(lo, hi + 1))
        x = (rng.normal(size=(frames, D)) * scale).astype(np.float32)
        post = []
        for _ in range(frames):
            k = int(rng.integers(1, min(3, G) + 1))
            w = rng.random(k) + 0.1
            post.append((rng.permutation(G)[:k].astype(np.int32), (w / w.sum()).astype(np.float32)))
        out.append((x, post))
    return out


def small_sums_elements(G, S):
    """what ivex_small_sums_kernel launches one thread for: gamma, ivector_sum, ivector_scatter and the objective"""
    return G + S + S * (S + 1) // 2 + 1


# (G, D, S) of the statistics' test: today's; the largest S whose elements fit one workgroup at G = 5 and the first that spills;
# and S = 70: eleven workgroups, the boundaries of gamma and ivector_sum inside the first one, and the last one with the
# objective alone (5 + 70 + 2485 elements fill ten workgroups to the brim)
_ONE_BLOCK_S = max(S for S in range(1, MAX_S) if small_sums_elements(5, S) <= TRAIN_THREADS)
STATS_CASES = [(7, 9, 11), (5, 7, _ONE_BLOCK_S), (5, 7, _ONE_BLOCK_S + 1), (5, 7, 70)]
SPLIT_SHAPE, SPLIT_UTTS = (5, 7, 2 * WAVE + 1), SLOTS + 2   # more than one flush, more than two waves of the posterior kernel
