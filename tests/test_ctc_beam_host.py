"""No GPU: the oracle of the CTC prefix beam search (tests/ctc_beam_oracle.py) against the exact CTC log-likelihood where the beam
holds every prefix, and the plumbing of `strategy: beam_batch` -- accepted by the three model classes, `beam` still refused,
language-model keys / timestamps / confidences refused by name, the ABI symbols exported and declared."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import ctc_beam_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_is_exact_where_the_beam_holds_every_prefix(seed):
    """T = 4, C = 3 (labels 0, 1 and the blank), W = 64, no pruning: all 15 label sequences that 4 frames can spell come out, each
    with its exact CTC log-likelihood, and their probabilities sum to 1"""
    lp = O.make_logp(seed, 4, 3)
    r = O.beam_search(lp, 2, 64)
    feasible = [p for U in range(5) for p in itertools.product((0, 1), repeat=U) if np.isfinite(O.ctc_loglik(lp, list(p), 2))]
    assert len(feasible) == 15 and sorted(p for p, _ in r["nbest"]) == sorted(feasible)
    assert r["margin"] == np.inf   # nothing was ever cut
    scores = [s for _, s in r["nbest"]]
    assert scores == sorted(scores, reverse=True)
    for p, s in r["nbest"]:
        assert abs(float(s) - O.ctc_loglik(lp, list(p), 2)) <= 1e-12, p
    assert abs(sum(np.exp(float(s)) for s in scores) - 1.0) <= 1e-6


def test_oracle_merges_an_extension_into_the_prefix_it_spells():
    """two frames that favour label 0: the prefix (0,) of frame 1 receives at frame 2 its stay AND the extension of the empty
    prefix by 0; without the merge its score would miss one of the three alignments (0 0, 0 _, _ 0)"""
    lp = np.log(np.array([[0.6, 0.1, 0.3], [0.5, 0.2, 0.3]], dtype=np.float32))
    r = dict(O.beam_search(lp, 2, 8)["nbest"])
    p = np.exp(lp.astype(np.float64))
    assert abs(np.exp(float(r[(0,)])) - (p[0, 0] * p[1, 0] + p[0, 0] * p[1, 2] + p[0, 2] * p[1, 0])) <= 1e-12
    # the float32 restatement differs from float64 by rounding only, and W = 1 keeps one hypothesis
    r32 = dict(O.beam_search(lp, 2, 8, dtype=np.float32)["nbest"])
    assert set(r32) == set(r) and all(abs(float(r32[k]) - float(r[k])) < 1e-5 for k in r)
    assert len(O.beam_search(lp, 2, 1)["nbest"]) == 1


def test_oracle_pruning_bonus_and_margin():
    lp = O.make_logp(5, 12, 9)
    full = O.beam_search(lp, 8, 4)
    assert np.isfinite(full["margin"]) and full["margin"] >= 0 and full["min_candidates"] > 4
    # a threshold of 1e-3 considers the arg-max class alone: the greedy label sequence, one hypothesis
    arg = lp.argmax(1).tolist()
    greedy = tuple(c for i, c in enumerate(arg) if c != 8 and (i == 0 or c != arg[i - 1]))
    one = O.beam_search(lp, 8, 4, theta=1e-3)
    assert [p for p, _ in one["nbest"]] == [greedy]
    # beta adds beta * len to every score of the same search when nothing is cut
    small = O.make_logp(5, 4, 3)   # (15 prefixes: W = 64 holds them all)
    a, b = O.beam_search(small, 2, 64), O.beam_search(small, 2, 64, beta=0.5)
    da, db = dict(a["nbest"]), dict(b["nbest"])
    assert set(da) == set(db) and all(abs(float(db[p]) - float(da[p]) - 0.5 * len(p)) < 1e-12 for p in da)


# ---------------------------------------------------------------------------------------------- config plumbing
def _ctc_cfg(**decoding):
    from nemo_amd.models import conformer_ctc_config
    cfg = conformer_ctc_config("small", vocab_size=len(VOCAB), d_model=32, n_heads=4, n_layers=1)
    cfg["decoder"]["vocabulary"] = VOCAB
    cfg["labels"] = VOCAB
    if decoding:
        cfg["decoding"] = decoding
    return cfg


def _hybrid_cfg(**decoding):
    from nemo_amd.models import fastconformer_hybrid_config
    cfg = fastconformer_hybrid_config("small", vocab_size=len(VOCAB), d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16)
    cfg["labels"] = VOCAB
    cfg["decoder"]["prednet"].update(pred_hidden=32, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=32, dropout=0.0)
    if decoding:
        cfg["aux_ctc"]["decoding"] = decoding
    return cfg


BEAM = dict(strategy="beam_batch", beam=dict(beam_size=4, return_best_hypothesis=False, beam_threshold=15.0, beam_beta=0.25))


def test_beam_batch_is_accepted_by_the_ctc_models():
    from nemo_amd.models import EncDecCTCModel
    from nemo_amd.modules import BeamBatchedCTCDecoder, GreedyCTCDecoder
    dec = EncDecCTCModel(_ctc_cfg(**BEAM)).wer.decoding
    assert isinstance(dec, BeamBatchedCTCDecoder)
    assert (dec.beam_size, dec.return_best_hypothesis, dec.beam_threshold, dec.beam_beta, dec.blank_id) == (4, False, 15.0, 0.25, len(VOCAB))
    dflt = EncDecCTCModel(_ctc_cfg(strategy="beam_batch")).wer.decoding
    assert (dflt.beam_size, dflt.return_best_hypothesis, dflt.beam_threshold, dflt.beam_beta) == (4, True, 20.0, 0.0)
    assert isinstance(EncDecCTCModel(_ctc_cfg()).wer.decoding, GreedyCTCDecoder)
    assert isinstance(EncDecCTCModel(_ctc_cfg(strategy="greedy")).wer.decoding, GreedyCTCDecoder)
    with pytest.raises(NotImplementedError, match="beam"):
        EncDecCTCModel(_ctc_cfg(strategy="beam", beam=dict(beam_size=4))).wer
    with pytest.raises(NotImplementedError, match="flashlight"):
        EncDecCTCModel(_ctc_cfg(strategy="flashlight")).wer


def test_beam_batch_is_accepted_by_the_bpe_model(tmp_path):
    from nemo_amd.models import EncDecCTCModelBPE
    from nemo_amd.modules import BeamBatchedCTCDecoder
    from test_abi_and_host import _train_spm
    words = ["hello", "world", "speech", "model", "conformer", "audio", "signal", "frame", "token", "layer", "attention", "gradient"]
    cfg = _ctc_cfg(**BEAM)
    cfg["decoder"].update(vocabulary=None, num_classes=-1)
    cfg.pop("labels")
    cfg["tokenizer"] = dict(dir=_train_spm(tmp_path, "tok64", 64, words), type="bpe")
    m = EncDecCTCModelBPE(cfg)
    dec = m.wer.decoding
    assert isinstance(dec, BeamBatchedCTCDecoder) and dec.blank_id == 64 and dec.word_pieces and dec.beam_size == 4
    assert dec.ids_to_text(m.tokenizer.text_to_ids("hello world")) == "hello world"
    with pytest.raises(NotImplementedError, match="beam"):
        EncDecCTCModelBPE(dict(cfg, decoding=dict(strategy="beam", beam=dict(beam_size=4)))).wer


def test_beam_batch_is_accepted_by_the_hybrid_model():
    from nemo_amd.models import EncDecHybridRNNTCTCModel
    from nemo_amd.modules import BeamBatchedCTCDecoder, GreedyCTCDecoder
    m = EncDecHybridRNNTCTCModel(_hybrid_cfg(**BEAM))
    assert isinstance(m.ctc_decoding, BeamBatchedCTCDecoder) and m.ctc_decoding.beam_beta == 0.25 and m.cur_decoder == "rnnt"
    m = EncDecHybridRNNTCTCModel(_hybrid_cfg())
    assert isinstance(m.ctc_decoding, GreedyCTCDecoder)
    m.change_decoding_strategy(dict(strategy="beam_batch", beam=dict(beam_size=7)), decoder_type="ctc")
    assert m.cur_decoder == "ctc" and isinstance(m.ctc_decoding, BeamBatchedCTCDecoder) and m.ctc_decoding.beam_size == 7
    assert m._text_decoding() is not None
    m.change_decoding_strategy(dict(strategy="greedy"), decoder_type="ctc")
    assert isinstance(m.ctc_decoding, GreedyCTCDecoder)
    with pytest.raises(NotImplementedError, match="beam"):
        m.change_decoding_strategy(dict(strategy="beam"), decoder_type="ctc")
    with pytest.raises(NotImplementedError, match="beam"):
        EncDecHybridRNNTCTCModel(_hybrid_cfg(strategy="beam"))
    with pytest.raises(NotImplementedError, match="ngram_lm_model"):   # refused before anything is replaced
        m.change_decoding_strategy(dict(strategy="beam_batch", beam=dict(ngram_lm_model="lm.arpa")), decoder_type="ctc")
    assert isinstance(m.ctc_decoding, GreedyCTCDecoder)


@pytest.mark.parametrize("beam,name", [(dict(ngram_lm_model="lm.arpa"), "ngram_lm_model"), (dict(kenlm_path="lm.bin"), "kenlm_path"),
                                       (dict(ngram_lm_alpha=0.3), "ngram_lm_alpha")])
def test_language_model_keys_are_refused_by_name(beam, name):
    from nemo_amd.models import EncDecCTCModel, EncDecHybridRNNTCTCModel
    from nemo_amd.modules import ctc_decoder_from_config
    with pytest.raises(NotImplementedError, match=name):
        EncDecCTCModel(_ctc_cfg(strategy="beam_batch", beam=beam)).wer
    with pytest.raises(NotImplementedError, match=name):
        EncDecHybridRNNTCTCModel(_hybrid_cfg(strategy="beam_batch", beam=beam))
    # unset / zero values of the same keys are the reference's defaults and pass
    dec = ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(ngram_lm_model=None, kenlm_path=None, ngram_lm_alpha=0.0)), VOCAB)
    assert dec.beam_size == 4


def test_timestamps_and_confidence_are_refused_by_name():
    from nemo_amd.models import EncDecCTCModel, EncDecHybridRNNTCTCModel
    conf = dict(preserve_token_confidence=True)
    with pytest.raises(NotImplementedError, match="confidence_cfg"):
        EncDecCTCModel(_ctc_cfg(strategy="beam_batch", confidence_cfg=conf)).wer
    with pytest.raises(NotImplementedError, match="confidence_cfg"):
        EncDecHybridRNNTCTCModel(_hybrid_cfg(strategy="beam_batch", confidence_cfg=conf))
    assert EncDecCTCModel(_ctc_cfg(strategy="beam_batch", confidence_cfg=dict(preserve_token_confidence=False))).wer is not None
    # timestamps=True is refused before any audio is touched
    m = EncDecCTCModel(_ctc_cfg(**BEAM))
    with pytest.raises(NotImplementedError, match="timestamps"):
        m.transcribe([np.zeros(1600, dtype=np.float32)], timestamps=True)
    h = EncDecHybridRNNTCTCModel(_hybrid_cfg(**BEAM))
    h.change_decoding_strategy(decoder_type="ctc")
    with pytest.raises(NotImplementedError, match="timestamps"):
        h.transcribe([np.zeros(1600, dtype=np.float32)], timestamps=True)


def test_decoder_arguments_are_checked():
    from nemo_amd.modules import BeamBatchedCTCDecoder, GreedyCTCDecoder
    for bad in (0, 65):
        with pytest.raises(ValueError, match="beam_size"):
            BeamBatchedCTCDecoder(VOCAB, beam_size=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="beam_threshold"):
            BeamBatchedCTCDecoder(VOCAB, beam_threshold=bad)
    with pytest.raises(ValueError, match="vocabulary or a blank_id"):
        BeamBatchedCTCDecoder()
    d = BeamBatchedCTCDecoder(blank_id=5, beam_size=64, beam_threshold=float("inf"))
    assert d.blank_id == 5 and d.vocabulary is None and d.confidence_cfg is None
    # the greedy decoder's surface is what it was
    g = GreedyCTCDecoder(VOCAB)
    assert g.blank_id == len(VOCAB) and g.ids_to_text([7, 8]) == "hi" and not g.word_pieces and g.confidence_cfg is None
    assert g.offsets([7], [2], [3])[0] == [{"char": "h", "start_offset": 2, "end_offset": 4}]


def test_beam_symbols_are_exported_declared_and_check_their_arguments():
    from nemo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    declared = set(re.findall(r"\b(mi355x_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mi355x_ctc_beam_decode", "mi355x_ctc_beam_workspace_elems"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["mi355x_ctc_beam_decode"]) == 16
    elems = _lib.lib.mi355x_ctc_beam_workspace_elems
    assert elems(501, 64) == 2 * 501 * 64 and elems(7, 1) == 14 and elems(10, 0) == 0 and elems(10, 65) == 0 and elems(0, 4) == 0
    # argument checks return MI_ERR_ARG (1) before anything is launched: the pointers are never followed
    p = 4096   # non-null, 8-byte aligned
    ok = dict(logp=p, lens=p, ws=p, tokens=p, tok_frame=p, hyp_len=p, score=p, n_hyp=p, B=2, T=8, C=5, blank=4, beam=4, thr=20.0, beta=0.0)

    def rc(**kw):
        a = dict(ok, **kw)
        return _lib.lib.mi355x_ctc_beam_decode(a["logp"], a["lens"], a["ws"], a["tokens"], a["tok_frame"], a["hyp_len"], a["score"],
                                               a["n_hyp"], a["B"], a["T"], a["C"], a["blank"], a["beam"], a["thr"], a["beta"], None)
    for ptr in ("logp", "lens", "ws", "tokens", "tok_frame", "hyp_len", "score", "n_hyp"):
        assert rc(**{ptr: None}) == 1, ptr
    for bad in (dict(beam=0), dict(beam=65), dict(beam=-1), dict(blank=-1), dict(blank=5), dict(thr=0.0), dict(thr=-1.0),
                dict(thr=float("nan")), dict(B=0), dict(T=0), dict(C=0), dict(C=8193, blank=0), dict(ws=p + 4)):
        assert rc(**bad) == 1, bad
