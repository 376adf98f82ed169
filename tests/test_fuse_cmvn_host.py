"""The recogniser of the per-speaker feature pipeline (csrc/fuse_pipe.h RecognizeCmvnPipeline through xv_recognize_cmvn_pipeline),
no GPU: the strings of the reference's acoustic-model scripts are taken apart field by field, everything that is not exactly that
pipeline is refused, and no string is claimed by both recognisers."""
import pytest

import helpers as H

S = "/data/split4/2"
BN_EMPTY = "ark,s,cs:apply-cmvn  --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (S, S, S)          # extract_bn.sh:59, $cmvn_opts empty
BN_OPTS = "ark,s,cs:apply-cmvn --norm-means=true --norm-vars=true --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (S, S, S)
AM_EMB = "ark:apply-cmvn --norm-means=true --norm-vars=false --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |" % (S, S, S)  # extract_am_embedding.sh:67
WITH_VAD = ("ark:apply-cmvn --norm-vars=false --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- | "
            "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (S, S, S, S))
GLOBAL = "ark:apply-cmvn --norm-vars=true /exp/global_cmvn.stats scp:%s/feats.scp ark:- |" % S
PER_UTT = "ark,s,cs:apply-cmvn ark:%s/cmvn_utt.ark ark:%s/feats.ark ark:- |" % (S, S)
WITH_PATH = "ark,s,cs:/opt/kaldi/src/featbin/apply-cmvn --norm_vars=true --utt2spk=ark:%s/utt2spk scp:%s/cmvn.scp scp:%s/feats.scp ark:- |  " % (S, S, S)
SLIDING = ("ark:apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 scp:%s/feats.scp ark:- | "
           "select-voiced-frames ark:- scp,s,cs:%s/vad.scp ark:- |" % (S, S))

ACCEPTED = {
    "extract_bn_empty_opts": (BN_EMPTY, dict(stats="scp:%s/cmvn.scp" % S, feats="scp:%s/feats.scp" % S, vad="", utt2spk="ark:%s/utt2spk" % S,
                                             **{"stats-is-table": "true", "norm-means": "true", "norm-vars": "false"})),
    "extract_bn_with_opts": (BN_OPTS, dict(stats="scp:%s/cmvn.scp" % S, feats="scp:%s/feats.scp" % S, vad="", utt2spk="ark:%s/utt2spk" % S,
                                           **{"stats-is-table": "true", "norm-means": "true", "norm-vars": "true"})),
    "extract_am_embedding": (AM_EMB, dict(stats="scp:%s/cmvn.scp" % S, feats="scp:%s/feats.scp" % S, vad="", utt2spk="ark:%s/utt2spk" % S,
                                          **{"stats-is-table": "true", "norm-means": "true", "norm-vars": "false"})),
    "with_select_voiced_frames": (WITH_VAD, dict(stats="scp:%s/cmvn.scp" % S, feats="scp:%s/feats.scp" % S, vad="scp,s,cs:%s/vad.scp" % S,
                                                 utt2spk="ark:%s/utt2spk" % S,
                                                 **{"stats-is-table": "true", "norm-means": "true", "norm-vars": "false"})),
    "global_stats_file": (GLOBAL, dict(stats="/exp/global_cmvn.stats", feats="scp:%s/feats.scp" % S, vad="", utt2spk="",
                                       **{"stats-is-table": "false", "norm-means": "true", "norm-vars": "true"})),
    "no_utt2spk": (PER_UTT, dict(stats="ark:%s/cmvn_utt.ark" % S, feats="ark:%s/feats.ark" % S, vad="", utt2spk="",
                                 **{"stats-is-table": "true", "norm-means": "true", "norm-vars": "false"})),
    "path_and_underscore": (WITH_PATH, dict(stats="scp:%s/cmvn.scp" % S, feats="scp:%s/feats.scp" % S, vad="", utt2spk="ark:%s/utt2spk" % S,
                                            **{"stats-is-table": "true", "norm-means": "true", "norm-vars": "true"})),
    "norm_means_false": (BN_EMPTY.replace("apply-cmvn ", "apply-cmvn --norm-means=false"),
                         dict(stats="scp:%s/cmvn.scp" % S, feats="scp:%s/feats.scp" % S, vad="", utt2spk="ark:%s/utt2spk" % S,
                              **{"stats-is-table": "true", "norm-means": "false", "norm-vars": "false"})),
}

T = "ark:apply-cmvn %%s --utt2spk=ark:%s/utt2spk %%s %%s ark:- |%%s" % S
STATS, FEATS = "scp:%s/cmvn.scp" % S, "scp:%s/feats.scp" % S
SELECT = " select-voiced-frames ark:- %s ark:- |"
REFUSED = {
    "skip_dims": T % ("--skip-dims=0", STATS, FEATS, ""),
    "reverse": T % ("--reverse=true", STATS, FEATS, ""),
    "verbose": T % ("--verbose=1", STATS, FEATS, ""),
    "config": T % ("--config=/c/cmvn.conf", STATS, FEATS, ""),
    "norm_vars_not_a_boolean": T % ("--norm-vars=maybe", STATS, FEATS, ""),
    "option_without_value": T % ("--norm-vars", STATS, FEATS, ""),
    "stats_from_stdin": T % ("", "ark:-", FEATS, ""),
    "stats_file_is_stdin": T % ("", "-", FEATS, ""),
    "stats_from_a_command": T % ("", "ark:copy-matrix scp:%s/cmvn.scp ark:- |" % S, FEATS, ""),
    "feats_from_stdin": T % ("", STATS, "ark:-", ""),
    "feats_from_a_command": T % ("", STATS, "ark:copy-feats scp:%s/feats.scp ark:- |" % S, ""),
    "feats_not_a_table": T % ("", STATS, "%s/feats.ark" % S, ""),
    "vad_from_stdin": T % ("", STATS, FEATS, SELECT % "ark:-"),
    "vad_from_a_command": T % ("", STATS, FEATS, SELECT % ("ark:copy-vector scp:%s/vad.scp ark:- |" % S)),
    "utt2spk_from_stdin": "ark:apply-cmvn --utt2spk=ark:- %s %s ark:- |" % (STATS, FEATS),
    "utt2spk_is_an_scp": "ark:apply-cmvn --utt2spk=scp:%s/utt2spk %s %s ark:- |" % (S, STATS, FEATS),
    "output_to_a_file": "ark:apply-cmvn %s %s ark:/tmp/out.ark |" % (STATS, FEATS),
    "third_stage": T % ("", STATS, FEATS, (SELECT % ("scp:%s/vad.scp" % S)) + " copy-feats ark:- ark:- |"),
    "second_stage_is_another_program": T % ("", STATS, FEATS, " copy-feats ark:- ark:- |"),
    "another_program": "ark:apply-cmvn-online %s %s ark:- |" % (STATS, FEATS),
    "compute_cmvn_stats": "ark:compute-cmvn-stats %s ark:- |" % FEATS,
    "single_quote": "ark:apply-cmvn --utt2spk='ark:%s/utt2spk' %s %s ark:- |" % (S, STATS, FEATS),
    "double_quote": 'ark:apply-cmvn "--utt2spk=ark:%s/utt2spk" %s %s ark:- |' % (S, STATS, FEATS),
    "dollar": "ark:apply-cmvn --utt2spk=ark:$sdata/utt2spk %s %s ark:- |" % (STATS, FEATS),
    "backquote": "ark:apply-cmvn `cat opts` %s %s ark:- |" % (STATS, FEATS),
    "semicolon": "ark:apply-cmvn %s %s ark:- ; true |" % (STATS, FEATS),
    "redirection": "ark:apply-cmvn %s %s ark:- 2>/dev/null |" % (STATS, FEATS),
    "newline": "ark:apply-cmvn %s %s\n ark:- |" % (STATS, FEATS),
    "no_trailing_bar": BN_EMPTY.rstrip("|").rstrip(),
    "scp_prefix": "scp:" + BN_EMPTY[len("ark,s,cs:"):],
    "unknown_option_letter": "ark,x:" + BN_EMPTY[len("ark,s,cs:"):],
    "not_a_pipe": "scp:%s/feats.scp" % S,
    "two_positionals": "ark:apply-cmvn %s ark:- |" % FEATS,
    "four_positionals": "ark:apply-cmvn %s %s %s ark:- |" % (STATS, FEATS, FEATS),
    "option_behind_a_positional": "ark:apply-cmvn %s --norm-vars=true %s ark:- |" % (STATS, FEATS),
    "empty": "",
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_the_scripts_strings_are_recognised(name):
    text, want = ACCEPTED[name]
    got = H.pkg().recognize_cmvn_pipeline(text)
    assert got == want, (text, got)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_anything_else_is_refused(name):
    assert H.pkg().recognize_cmvn_pipeline(REFUSED[name]) is None, REFUSED[name]


def test_no_string_is_claimed_by_both_recognisers():
    P = H.pkg()
    for name, (text, _) in ACCEPTED.items():
        assert P.recognize_feature_pipeline(text) is None, name
    assert P.recognize_feature_pipeline(SLIDING) is not None
    for text in (SLIDING, SLIDING.split(" | ")[0] + " |"):
        assert P.recognize_cmvn_pipeline(text) is None, text
    # the sliding recogniser keeps its "ark:" prefix to itself
    assert P.recognize_feature_pipeline("ark,s,cs:" + SLIDING[4:]) is None
