"""CPU tests of tests/nnet2_ref.py, the restatement the GPU tests of nnet-am-compute compare with: hand-computed values for every
piece whose definition could be read two ways."""
import numpy as np

import nnet2_ref as R


def test_one_pnorm_group_is_the_two_norm_of_its_inputs():
    x = np.array([[3.0, 4.0, 1.0, 2.0, 2.0, 0.0]])
    assert np.array_equal(R.pnorm(x, 2), [[np.sqrt(26.0), np.sqrt(8.0)]])     # groups of consecutive inputs: (3, 4, 1), (2, 2, 0)
    assert np.array_equal(R.pnorm(x, 3), [[5.0, np.sqrt(5.0), 2.0]])
    assert np.array_equal(R.pnorm(x, 6), np.abs(x))


def test_normalize_gives_unit_mean_square_and_floors_an_all_zero_row():
    y = R.normalize(np.array([[3.0, 4.0], [0.0, 0.0], [2.0 ** -40, 0.0]]))
    assert np.allclose(y[0], np.array([3.0, 4.0]) / np.sqrt(12.5), rtol=1e-15)
    assert np.array_equal(y[1], [0.0, 0.0])                                   # 0 * 2^33, not 0 / 0
    assert y[2, 0] == 2.0 ** -40 * 2.0 ** 33                                   # mean square 2^-81 is under the floor 2^-66
    assert R.normalize(np.zeros((1, 4), np.float32)).dtype == np.float32


def test_softmax_floors_what_underflows():
    p = R.softmax(np.array([[0.0, -100.0, np.log(3.0)]]))
    assert np.allclose(p[0, [0, 2]], [0.25, 0.75], rtol=1e-15) and p[0, 1] == 1e-20   # exp(-100) / 4 = 9e-45
    assert np.array_equal(R.softmax(np.array([[1000.0, 1000.0]])), [[0.5, 0.5]])       # the maximum is subtracted first


def test_sum_group_of_sizes_1_3_1():
    x = np.array([[1.0, 2.0, 4.0, 8.0, 16.0], [0.5, 0.25, 0.25, 0.5, 1.0]])
    assert np.array_equal(R.sum_group(x, [1, 3, 1]), [[1.0, 14.0, 16.0], [0.5, 1.0, 1.0]])


def test_splice_concatenates_in_context_order():
    x = np.arange(12.0).reshape(6, 2)
    s = R.splice(x, [-1, 2])
    assert s.shape == (3, 4) and np.array_equal(s[0], [0, 1, 6, 7]) and np.array_equal(s[2], [4, 5, 10, 11])


def test_padding_a_one_frame_utterance_repeats_it():
    x = np.array([[1.0, 2.0]])
    assert np.array_equal(R.pad(x, 3, 2), np.tile(x, (6, 1)))
    comps = [("Splice", 2, [-1, 0, 1]), ("Affine", np.array([[1.0, 0, 1.0, 0, 1.0, 0], [0, 1.0, 0, 1.0, 0, 1.0]]), np.zeros(2)), ("Softmax", 2)]
    out = R.forward(comps, (), x)                                               # logits (3, 6)
    assert out.shape == (1, 2) and np.allclose(out[0, 0], 1.0 / (1.0 + np.exp(3.0)), rtol=1e-12)
    assert R.forward(comps, (), x, pad_input=False) is None and R.forward(comps, (), np.zeros((3, 2)), pad_input=False).shape == (1, 2)
    assert R.forward(comps, (), np.zeros((0, 2))) is None


def test_priors_and_log_come_last_and_the_recipe_s_contexts_are_13_and_9():
    comps, priors = R.miniature()
    assert R.contexts(comps) == (13, 9)
    x = np.random.default_rng(1).normal(size=(5, 8))
    post = R.forward(comps, priors, x)
    assert post.shape == (5, 17) and np.allclose(post.sum(axis=1), 1.0, rtol=1e-12)
    both = R.forward(comps, priors, x, apply_log=True, divide_by_priors=True)
    assert np.allclose(both, np.log(post / priors.astype(np.float64)), rtol=1e-12)
    f32 = R.forward(comps, priors, x, np.float32, apply_log=True)
    assert f32.dtype == np.float32 and np.abs(f32 - np.log(post)).max() < 1e-4


def test_binary_and_text_models_hold_the_same_components():
    comps, priors = R.miniature()
    b, t = R.model_bytes(comps, priors, True), R.model_bytes(comps, priors, False)
    assert b[:2] == b"\0B" and b"<Context>" in b and t.lstrip().startswith(b"<TransitionModel>")
    rb = R.model_bytes(*R.relu_model())
    assert b"</RectifiedLinearComponent>" in rb and R.contexts(R.relu_model()[0]) == (2, 1)
    for blob in (b, t):
        for name in ("SpliceComponent", "FixedAffineComponent", "AffineComponent", "AffineComponentPreconditioned",
                     "AffineComponentPreconditionedOnline", "PnormComponent", "NormalizeComponent", "SoftmaxComponent", "SumGroupComponent"):
            assert ("</%s>" % name).encode() in blob


def test_the_pipeline_case_s_seed_keeps_the_restatement_within_two_percent():
    """The GPU test of the shell pipeline leaves out frames where a reference posterior lies within the tolerance of
    --min-post=0.025, and asserts that these are at most 2 %; with this seed the fp32 restatement alone stays within that, and
    agrees with float64 on every other frame."""
    comps, priors, utts, vads = R.pipeline_case()
    left_out = total = 0
    for (_, x), (_, v) in zip(utts, vads):
        p64 = np.exp(R.forward(comps, priors, x, apply_log=True))
        l32 = R.forward(comps, priors, x, np.float32, apply_log=True)
        tol = R.tolerance(R.forward(comps, priors, x, apply_log=True), l32) * p64   # an error of the logarithm, as one of the posterior
        near = R.near_threshold(p64, tol, v)
        a, b = R.kept_sets(p64, v), R.kept_sets(np.exp(l32.astype(np.float64)), v)
        assert all(x_ == y_ for x_, y_, n in zip(a, b, near) if not n)
        left_out += int(near.sum())
        total += len(near)
    assert total > 100 and left_out <= 0.02 * total
    assert sum(len(s) for s in a) > len(a)   # more than one senone per frame reaches the threshold: the posteriors are not flat, nor one-hot
