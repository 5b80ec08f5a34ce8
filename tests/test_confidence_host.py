"""No GPU: the confidence measures' float64 restatement (tests/confidence_oracle.py) at its fixed points, and the host side of
confidence estimation (nemo_amd/modules/confidence.py): configuration objects and their validation, the constants handed to the
kernels, aggregation, word grouping, and the declarations of the five entry points."""
import math
import os
import re

import numpy as np
import pytest

import confidence_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = [("max_prob", "tsallis"), ("entropy", "gibbs"), ("entropy", "tsallis"), ("entropy", "renyi")]
ALPHAS = [0.33, 0.5, 1.0, 2.0]
SIZES = [2, 37, 1025]


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("norm", ["lin", "exp"])
@pytest.mark.parametrize("name,etype", METHODS)
def test_oracle_gives_one_for_one_hot_and_zero_for_uniform(name, etype, norm, alpha, V):
    cfg = CO.Method(name, etype, alpha, norm)
    hot_inf = np.full((2, V), -np.inf)
    hot_inf[0, 0] = 0.0
    hot_inf[1, V - 1] = 0.0
    hot_far = np.full((1, V), -800.0)    # a one-hot row whose other entries are merely negligible
    hot_far[0, V // 2] = 0.0
    uniform = np.full((1, V), -math.log(V))
    with np.errstate(invalid="raise"):   # a -inf class must not turn into 0 * inf
        assert np.abs(CO.frame_confidence(hot_inf, cfg) - 1.0).max() <= 1e-12
    assert abs(float(CO.frame_confidence(hot_far, cfg)[0]) - 1.0) <= 1e-12
    assert abs(float(CO.frame_confidence(uniform, cfg)[0])) <= 1e-12


@pytest.mark.parametrize("norm", ["lin", "exp"])
@pytest.mark.parametrize("etype", ["tsallis", "renyi"])
def test_tsallis_and_renyi_at_alpha_one_are_gibbs(etype, norm):
    rng = np.random.default_rng(3)
    z = rng.standard_normal((9, 37)) * 3
    logp = z - np.log(np.exp(z).sum(-1, keepdims=True))
    got = CO.frame_confidence(logp, CO.Method("entropy", etype, 1.0, norm))
    want = CO.frame_confidence(logp, CO.Method("entropy", "gibbs", 1.0, norm))
    assert np.array_equal(got, want)
    # and between the fixed points the measure is strictly inside (0, 1) and orders a sharp row above a flat one
    sharp, flat = np.log(np.array([0.97] + [0.03 / 36] * 36)), np.log(np.array([0.1] + [0.9 / 36] * 36))
    cs, cf = (float(CO.frame_confidence(r[None], CO.Method("entropy", etype, 1.0, norm))[0]) for r in (sharp, flat))
    assert 0.0 < cf < cs < 1.0


def test_config_validation():
    from nemo_amd.modules import ConfidenceConfig, ConfidenceMethodConfig, confidence_from
    d = ConfidenceMethodConfig()
    assert (d.name, d.entropy_type, d.alpha, d.entropy_norm) == ("entropy", "tsallis", 0.33, "exp")
    c = ConfidenceConfig()
    assert (c.aggregation, c.exclude_blank) == ("min", True)
    assert not (c.preserve_frame_confidence or c.preserve_token_confidence or c.preserve_word_confidence)
    assert confidence_from(None) is None and confidence_from({}) is None   # nothing asked for: no confidence path
    c = ConfidenceConfig.from_dict({"preserve_word_confidence": True, "aggregation": "prod", "exclude_blank": False,
                                    "method_cfg": {"name": "entropy", "entropy_type": "renyi", "alpha": 0.5, "entropy_norm": "lin"}})
    assert isinstance(c.method_cfg, ConfidenceMethodConfig) and c.method_cfg.entropy_type == "renyi" and c.method_cfg.alpha == 0.5
    assert c.aggregation == "prod" and c.exclude_blank is False and confidence_from(c) is c
    for bad in ({"name": "margin"}, {"entropy_type": "shannon"}, {"entropy_norm": "log"}, {"alpha": 0.0}, {"alpha": -1.0},
                {"temperature": 1.0}):
        with pytest.raises(ValueError):
            ConfidenceMethodConfig.from_dict(bad)
    for bad in ({"aggregation": "median"}, {"method_cfg": {"alpha": 0}}, {"preserve_all": True}):
        with pytest.raises(ValueError):
            ConfidenceConfig.from_dict(bad)
    with pytest.raises(ValueError):
        ConfidenceMethodConfig().constants(1)


def test_aggregate():
    from nemo_amd.modules import aggregate
    v = [0.5, 0.25, 1.0, 0.8]
    assert aggregate(v, "mean") == pytest.approx(0.6375, abs=1e-15)
    assert aggregate(v, "min") == 0.25 and aggregate(v, "max") == 1.0
    assert aggregate(v, "prod") == pytest.approx(0.1, abs=1e-15)
    assert aggregate([0.7], "prod") == 0.7
    with pytest.raises(ValueError):
        aggregate(v, "median")
    with pytest.raises(ValueError):
        aggregate([], "min")


def test_word_confidence_follows_the_grouping_of_ctc_offsets():
    from nemo_amd.modules import ctc_offsets, word_confidence
    # word pieces: a leading U+2581 starts a word; the first token starts one in any case
    toks = ["he", "llo", "▁wor", "ld", "▁", "a", "▁b"]
    conf = [0.9, 0.5, 0.8, 0.6, 0.3, 0.7, 0.2]
    assert [w["word"] for w in ctc_offsets(toks, range(7), range(7), word_pieces=True)[1]] == ["hello", "world", "a", "b"]
    assert word_confidence(toks, conf, True, "min") == [0.5, 0.6, 0.3, 0.2]
    assert word_confidence(toks, conf, True, "max") == [0.9, 0.8, 0.7, 0.2]
    assert word_confidence(toks, conf, True, "mean") == pytest.approx([0.7, 0.7, 0.5, 0.2], abs=1e-15)
    assert word_confidence(toks, conf, True, "prod") == pytest.approx([0.45, 0.48, 0.21, 0.2], abs=1e-15)
    # characters: the space token separates words and belongs to none
    chars = [" ", "h", "i", " ", " ", "y", "o", "u", " "]
    cc = [0.01, 0.9, 0.8, 0.02, 0.03, 0.5, 0.6, 0.7, 0.04]
    assert [w["word"] for w in ctc_offsets(chars, range(9), range(9))[1]] == ["hi", "you"]
    assert word_confidence(chars, cc, False, "min") == [0.8, 0.5]
    assert word_confidence(chars, cc, False, "prod") == pytest.approx([0.72, 0.21], abs=1e-15)
    assert word_confidence(chars, cc, False, "mean") == pytest.approx([0.85, 0.6], abs=1e-15)
    assert word_confidence([], [], True, "min") == []


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("norm", ["lin", "exp"])
@pytest.mark.parametrize("name,etype", METHODS)
def test_host_constants_equal_the_oracles(name, etype, norm, alpha, V):
    from nemo_amd.modules import ConfidenceMethodConfig
    cfg = ConfidenceMethodConfig(name=name, entropy_type=etype, alpha=alpha, entropy_norm=norm)
    assert cfg.constants(V) == CO.constants(V, cfg)
    assert cfg.method == CO.method_row(cfg)
    m, n, a, k0, k1, k2 = cfg.kernel_args(V)
    assert m == {"max_prob": 0, "gibbs": 1, "tsallis": 2, "renyi": 3}[CO.method_row(cfg)] and n == {"lin": 0, "exp": 1}[norm]
    assert (a, k0, k1, k2) == (alpha,) + CO.constants(V, cfg)


def test_an_alpha_that_rounds_to_one_in_float_takes_the_alpha_one_row_on_both_sides():
    from nemo_amd.modules import ConfidenceMethodConfig
    for etype in ("tsallis", "renyi", "gibbs"):
        near = ConfidenceMethodConfig(entropy_type=etype, alpha=1.0 + 1e-9)   # the kernel sees alpha == 1.0f
        assert near.method == "gibbs" and near.kernel_args(37)[0] == 1 and near.kernel_args(37)[5] == 0.0
        away = ConfidenceMethodConfig(entropy_type=etype, alpha=1.0 + 1e-6)
        assert away.method == etype


def test_the_new_entry_points_are_declared():
    from nemo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    declared = set(re.findall(r"\bint (mi355x_[a-z0-9_]+)\s*\(", hdr))
    for name in ("mi355x_ctc_greedy_decode_conf", "mi355x_transducer_greedy_decode"):   # (the transducer searches: one entry)
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name), name
    assert "mi355x_transducer_greedy_desc" in hdr and "mi355x_transducer_conf" in hdr
    for macro, value in (("MI355X_CONF_MAX_PROB", 0), ("MI355X_CONF_GIBBS", 1), ("MI355X_CONF_TSALLIS", 2), ("MI355X_CONF_RENYI", 3),
                         ("MI355X_CONF_NORM_LIN", 0), ("MI355X_CONF_NORM_EXP", 1), ("MI355X_CONF_AGG_MEAN", 0),
                         ("MI355X_CONF_AGG_MIN", 1), ("MI355X_CONF_AGG_MAX", 2), ("MI355X_CONF_AGG_PROD", 3)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro


def test_invalid_confidence_arguments_are_rejected_before_any_launch():
    from nemo_amd import _lib
    one = 1   # non-null stand-ins: validation comes first, nothing is dereferenced or launched
    ptrs = [one] * 9

    def call(C=37, blank=36, method=2, norm=1, alpha=0.33, agg=1, tok_conf=one):
        p = list(ptrs)
        p[8] = tok_conf
        return _lib.lib.mi355x_ctc_greedy_decode_conf(*p, 2, 8, C, blank, method, norm, alpha, 1.0, 1.0, 0.0, agg, 1, None)
    for kw in (dict(C=1, blank=0), dict(alpha=0.0), dict(alpha=-0.5), dict(method=4), dict(method=-1), dict(norm=2), dict(agg=4),
               dict(agg=-1), dict(tok_conf=None), dict(blank=37)):
        assert call(**kw) == 1, kw


@pytest.mark.parametrize("entry", ["rnnt", "tdt", "rnnt_stream", "tdt_stream"])
def test_invalid_confidence_arguments_of_the_searches_are_rejected_before_any_launch(entry):
    import ctypes as C
    from nemo_amd import _lib
    from nemo_amd.ops import _StreamStateC
    one, B, T, J, H, V1 = 1, 2, 8, 32, 32, 49   # non-null stand-ins and valid sizes: only the confidence arguments are wrong
    dur = (C.c_int * 5)(0, 1, 2, 3, 4)
    state = _StreamStateC(*([one] * 7))

    def call(tok_conf=one, method=2, norm=1, alpha=0.33):   # `entry` as descriptor settings of the one entry
        q = _lib.TransducerConf(method, norm, alpha, 1.0, 1.0, 0.0)
        d = _lib.TransducerGreedyDesc(
            enc_proj=one, f_dtype=0, ldf=J, enc_len=one, emb=one, w_ih=one, ld_ih=H, w_hh=one, ld_hh=H, b_ih=one, b_hh=one, w_pred=one,
            ld_pred=H, b_pred=one, w_out=one, ld_out=J, b_out=one, w_dtype=0, B=B, T=T, J=J, H=H, V1=V1, blank=V1 - 1, max_symbols=10,
            tokens=one, times=one, out_len=one, max_out=80, conf=C.addressof(q), tok_conf=tok_conf)
        if entry.startswith("tdt"):
            d.D, d.durations = 5, C.addressof(dur)
        if "stream" in entry:   # fresh streams; no score / h / c, as the resumable searches are called
            d.state_out = C.addressof(state)
        else:
            d.score = one
        return _lib.lib.mi355x_transducer_greedy_decode(C.byref(d), None)
    for kw in (dict(tok_conf=None), dict(alpha=0.0), dict(alpha=-1.0), dict(method=4), dict(method=-1), dict(norm=2), dict(norm=-1)):
        assert call(**kw) == 1, kw
