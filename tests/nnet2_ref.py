"""What the tests of nnet-am-compute compare with: a writer of nnet2 acoustic models as the reader of csrc/nnet2_model.h takes them
(binary and text, every supported component, both spellings of the splice), the forward pass of csrc/nnet2.h in float64, and the
same forward in float32 (the restatement whose own error sets the tolerance of the device tests).  numpy only.

A model is a list of components:
  ("Splice", input_dim, context[, legacy])   legacy: written as <LeftContext> / <RightContext> (the context must be contiguous)
  ("FixedAffine" | "Affine" | "AffinePreconditioned" | "AffinePreconditionedOnline", W [out, in], b [out][, single_rank])
  ("Pnorm", input_dim, output_dim[, p])
  ("RectifiedLinear" | "Normalize" | "Softmax", dim)
  ("SumGroup", sizes)
and a vector of priors (possibly empty)."""
import io
import struct

import numpy as np

from oracle import kaldi_io as K

AFFINE = ("FixedAffine", "Affine", "AffinePreconditioned", "AffinePreconditionedOnline")
RECIPE_SPLICES = ([-2, -1, 0, 1, 2], [-1, 2], None, [-3, 3], [-7, 2])   # local/dnn/run_nnet2_multisplice.sh:49
MIN_NORM = 2.0 ** -66
FLOOR = 1e-20


# ----------------------------------------------------------------------------------------------------------------------- the writer
def _int_vector(f, v, binary):
    if binary:
        f.write(b"\x04" + struct.pack("<i", len(v)) + np.asarray(v, "<i4").tobytes())
    else:
        f.write(("[ " + "".join("%d " % x for x in v) + "]\n").encode())


def _stats(f, dim, binary, double, empty):
    K.write_token(f, "<ValueSum>", binary)
    K.write_vector(f, np.zeros(0 if empty else dim), binary, double)
    K.write_token(f, "<DerivSum>", binary)
    K.write_vector(f, np.zeros(0 if empty else dim), binary, double)
    K.write_token(f, "<Count>", binary)
    (K.write_double if double else K.write_float)(f, 0.0, binary)


def write_component(f, comp, binary=True, index=0):
    kind = comp[0]
    name = {"AffinePreconditioned": "AffineComponentPreconditioned", "AffinePreconditionedOnline": "AffineComponentPreconditionedOnline"}.get(
        kind, kind + "Component")
    K.write_token(f, "<%s>" % name, binary)
    if kind == "Splice":
        _, dim, context = comp[:3]
        legacy = len(comp) > 3 and comp[3]
        K.write_token(f, "<InputDim>", binary)
        K.write_int32(f, dim, binary)
        if legacy:
            assert list(context) == list(range(context[0], context[-1] + 1))
            K.write_token(f, "<LeftContext>", binary)
            K.write_int32(f, -context[0], binary)
            K.write_token(f, "<RightContext>", binary)
            K.write_int32(f, context[-1], binary)
        else:
            K.write_token(f, "<Context>", binary)
            _int_vector(f, context, binary)
        K.write_token(f, "<ConstComponentDim>", binary)
        K.write_int32(f, comp[4] if len(comp) > 4 else 0, binary)
    elif kind in AFFINE:
        _, w, b = comp[:3]
        if kind != "FixedAffine":
            K.write_token(f, "<LearningRate>", binary)
            K.write_float(f, 0.001, binary)
        K.write_token(f, "<LinearParams>", binary)
        K.write_matrix(f, np.asarray(w, np.float32), binary)
        K.write_token(f, "<BiasParams>", binary)
        K.write_vector(f, np.asarray(b, np.float32), binary)
        if kind == "Affine":
            K.write_token(f, "<IsGradient>", binary)
            K.write_bool(f, False, binary)
        elif kind == "AffinePreconditioned":
            for tok, v in (("<Alpha>", 4.0), ("<MaxChange>", 10.0)):
                K.write_token(f, tok, binary)
                K.write_float(f, v, binary)
        elif kind == "AffinePreconditionedOnline":
            for tok in (("<Rank>",) if len(comp) > 3 and comp[3] else ("<RankIn>", "<RankOut>")):
                K.write_token(f, tok, binary)
                K.write_int32(f, 20, binary)
            K.write_token(f, "<UpdatePeriod>", binary)
            K.write_int32(f, 4, binary)
            for tok, v in (("<NumSamplesHistory>", 2000.0), ("<Alpha>", 4.0), ("<MaxChangePerSample>", 0.075)):
                K.write_token(f, tok, binary)
                K.write_float(f, v, binary)
    elif kind == "Pnorm":
        for tok, v in (("<InputDim>", comp[1]), ("<OutputDim>", comp[2])):
            K.write_token(f, tok, binary)
            K.write_int32(f, v, binary)
        K.write_token(f, "<P>", binary)
        K.write_float(f, comp[3] if len(comp) > 3 else 2.0, binary)
    elif kind == "SumGroup":
        K.write_token(f, "<Sizes>", binary)
        _int_vector(f, comp[1], binary)
    elif kind in ("RectifiedLinear", "Normalize", "Softmax") or len(comp) == 2:   # also an unknown type with one dimension
        K.write_token(f, "<Dim>", binary)
        K.write_int32(f, comp[1], binary)
        _stats(f, comp[1], binary, double=index % 2 == 1, empty=index % 3 == 0)
    else:
        raise ValueError(kind)
    K.write_token(f, "</%s>" % name, binary)
    if not binary:
        f.write(b"\n")


def model_bytes(components, priors=(), binary=True):
    f = io.BytesIO()
    if binary:
        f.write(b"\0B")
    K.write_token(f, "<TransitionModel>", binary)
    K.write_token(f, "<Topology>", binary)
    K.write_token(f, "</Topology>", binary)
    K.write_token(f, "<Triples>", binary)
    K.write_int32(f, 0, binary)
    K.write_token(f, "</Triples>", binary)
    K.write_token(f, "<LogProbs>", binary)
    K.write_vector(f, np.zeros(1), binary)
    K.write_token(f, "</LogProbs>", binary)
    K.write_token(f, "</TransitionModel>", binary)
    if not binary:
        f.write(b"\n")
    K.write_token(f, "<Nnet>", binary)
    K.write_token(f, "<NumComponents>", binary)
    K.write_int32(f, len(components), binary)
    K.write_token(f, "<Components>", binary)
    if not binary:
        f.write(b"\n")
    for i, c in enumerate(components):
        write_component(f, c, binary, i)
    K.write_token(f, "</Components>", binary)
    K.write_token(f, "</Nnet>", binary)
    K.write_vector(f, np.asarray(priors, np.float32), binary)
    return f.getvalue()


def write_model(path, components, priors=(), binary=True):
    with open(path, "wb") as f:
        f.write(model_bytes(components, priors, binary))
    return path


# ------------------------------------------------------------------------------------------------------------------- model builders
def multisplice(rng, dim, lda_out, pnorm_in, pnorm_out, final, sizes=None, splices=RECIPE_SPLICES, extra_hidden=0, final_std=None,
                legacy_first=False):
    """The shape steps/nnet2/make_multisplice_configs.py gives: splice + LDA, one hidden layer on the LDA's output, one hidden layer
    per further entry of `splices` (None: no splice), extra_hidden more, the final affine, softmax and (sizes) the group sum of a
    mixed-up model.  Weights N(0, 1) / sqrt(pnorm_in), as the configs' param-stddev."""
    std = 1.0 / np.sqrt(pnorm_in)
    kinds = ("AffinePreconditionedOnline", "AffinePreconditioned", "Affine")
    comps = [("Splice", dim, list(splices[0]), legacy_first),
             ("FixedAffine", rng.normal(size=(lda_out, dim * len(splices[0]))) / np.sqrt(dim * len(splices[0])), rng.normal(size=lda_out) * 0.1)]
    width = lda_out
    for i, s in enumerate([None] + list(splices[1:]) + [None] * extra_hidden):
        k = width
        if s is not None:
            comps.append(("Splice", width, list(s)))
            k = width * len(s)
        comps += [(kinds[i % 3], rng.normal(size=(pnorm_in, k)) * std, rng.normal(size=pnorm_in) * std, i % 2 == 1),
                  ("Pnorm", pnorm_in, pnorm_out), ("Normalize", pnorm_out)]
        width = pnorm_out
    comps += [("AffinePreconditionedOnline", rng.normal(size=(final, width)) * (final_std or std), rng.normal(size=final) * std), ("Softmax", final)]
    if sizes is not None:
        comps.append(("SumGroup", [int(x) for x in sizes]))
    return comps


def random_sizes(rng, total, groups):
    """`groups` positive sizes summing to `total`"""
    cuts = np.sort(rng.choice(np.arange(1, total), size=groups - 1, replace=False))
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64)


def miniature(seed=0):
    """dim 8, the recipe's splices, LDA 40 -> 24, p-norm 60 -> 6, final 6 -> 37, sum-group -> 17: (components, priors)"""
    rng = np.random.default_rng(seed)
    comps = multisplice(rng, 8, 24, 60, 6, 37, random_sizes(rng, 37, 17), final_std=1.5)
    priors = rng.uniform(0.2, 1.0, size=17)
    return comps, (priors / priors.sum()).astype(np.float32)


def relu_model(seed=1):
    """A ReLU network, as train_multisplice_accel2.sh's other nonlinearity gives: splice, affine, ReLU, normalize; affine, ReLU
    (no normalize); affine, softmax.  dim 5 -> 12 outputs, contexts 2 and 1: (components, priors)"""
    rng = np.random.default_rng(seed)
    comps = [("Splice", 5, [-2, 0, 1]), ("Affine", rng.normal(size=(20, 15)) / np.sqrt(15), rng.normal(size=20) * 0.1), ("RectifiedLinear", 20),
             ("Normalize", 20), ("AffinePreconditioned", rng.normal(size=(9, 20)) / np.sqrt(20), rng.normal(size=9) * 0.1), ("RectifiedLinear", 9),
             ("AffinePreconditionedOnline", rng.normal(size=(12, 9)), rng.normal(size=12) * 0.1), ("Softmax", 12)]
    return comps, ()


def contexts(components):
    left = sum(-c[2][0] for c in components if c[0] == "Splice")
    right = sum(c[2][-1] for c in components if c[0] == "Splice")
    return left, right


# ---------------------------------------------------------------------------------------------------------------------- the forward
def splice(x, context):
    lo, hi = -context[0], context[-1]
    rows = x.shape[0] - lo - hi
    return np.concatenate([x[lo + c:lo + c + rows] for c in context], axis=1)


def pnorm(x, out_dim):
    g = x.shape[1] // out_dim
    return np.sqrt((x.reshape(x.shape[0], out_dim, g) ** 2).sum(axis=2))


def normalize(x):
    d = x.dtype.type
    ms = (x * x).sum(axis=1, keepdims=True) / d(x.shape[1])
    return x * (np.maximum(ms, d(MIN_NORM)) ** d(-0.5))


def softmax(x):
    d = x.dtype.type
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return np.maximum(e / e.sum(axis=1, keepdims=True), d(FLOOR))


def sum_group(x, sizes):
    start = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([x[:, start[g]:start[g + 1]].sum(axis=1) for g in range(len(sizes))], axis=1)


def pad(x, left, right):
    return np.concatenate([np.repeat(x[:1], left, axis=0), x, np.repeat(x[-1:], right, axis=0)], axis=0)


def forward(components, priors, feats, dtype=np.float64, apply_log=False, divide_by_priors=False, pad_input=True):
    """The output rows of one utterance ([T, dim]); None where the tool skips it (no rows; without padding, too few)."""
    left, right = contexts(components)
    x = np.asarray(feats, dtype=dtype)
    if x.shape[0] == 0 or (not pad_input and x.shape[0] <= left + right):
        return None
    if pad_input:
        x = pad(x, left, right)
    for c in components:
        kind = c[0]
        if kind == "Splice":
            x = splice(x, c[2])
        elif kind in AFFINE:
            x = x @ np.asarray(c[1], np.float32).astype(dtype).T + np.asarray(c[2], np.float32).astype(dtype)
        elif kind == "Pnorm":
            x = pnorm(x, c[2])
        elif kind == "RectifiedLinear":
            x = np.maximum(x, dtype(0))
        elif kind == "Normalize":
            x = normalize(x)
        elif kind == "Softmax":
            x = softmax(x)
        elif kind == "SumGroup":
            x = sum_group(x, c[1])
        else:
            raise ValueError(kind)
    if divide_by_priors:
        p = np.asarray(priors, np.float32)
        assert p.shape == (x.shape[1],)
        x = x * (dtype(1) / p.astype(dtype))
    if apply_log:
        x = np.log(np.maximum(x, dtype(FLOOR)))
    return x


def tolerance(ref64, ref32):
    """What a device value may differ from ref64 by, per row [rows, 1]: 8 x the largest error of the fp32 restatement on the same
    inputs, or 2^-21 of the row's largest magnitude where that is more (the split operands carry 22 of fp32's 24 bits: 4 x; the
    summation order: 2 x)."""
    err32 = np.abs(np.asarray(ref32, np.float64) - ref64).max()
    return np.maximum(8.0 * err32, 2.0 ** -21 * np.abs(ref64).max(axis=1, keepdims=True))


# ------------------------------------------------------------------------------------------------- the pipeline case of the tests
PIPELINE_SEED = 4
MIN_POST = 0.025


def pipeline_case(seed=PIPELINE_SEED):
    """The miniature network, three utterances and their voice-activity decisions, for
    nnet-am-compute --apply-log=true | select-voiced-frames | logprob-to-post --min-post=0.025: (components, priors, utts, vads)"""
    comps, priors = miniature(seed)
    rng = np.random.default_rng(seed + 100)
    utts = [("spk1-a", rng.normal(size=(120, 8)).astype(np.float32)), ("spk1-b", rng.normal(size=(40, 8)).astype(np.float32)),
            ("spk2-a", rng.normal(size=(77, 8)).astype(np.float32))]
    vads = [(k, (rng.uniform(size=len(x)) < 0.7).astype(np.float32)) for k, x in utts]
    return comps, priors, utts, vads


def kept_sets(post, voiced, min_post=MIN_POST):
    """per voiced frame the set of senones whose posterior reaches min_post (logprob-to-post --random-prune=false)"""
    return [frozenset(np.nonzero(row >= min_post)[0].tolist()) for row in np.asarray(post)[voiced > 0]]


def near_threshold(post64, tol, voiced, min_post=MIN_POST):
    """per voiced frame: whether a reference posterior lies within the tolerance of the threshold"""
    return (np.abs(post64 - min_post) <= tol).any(axis=1)[voiced > 0]
