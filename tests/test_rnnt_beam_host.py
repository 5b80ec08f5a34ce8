"""CPU-side checks of the transducer beam search (no kernel is launched): `strategy: malsd_batch` is read by the three places that
take a transducer decoding section, everything outside its scope is refused by name, and mi355x_transducer_beam_decode refuses bad
arguments before any launch."""
import ctypes

import pytest

VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


def _cfg(hybrid=False, tdt=False, layers=1, **decoding):
    from nemo_amd.models import fastconformer_hybrid_config, fastconformer_tdt_config, fastconformer_transducer_config
    make = fastconformer_hybrid_config if hybrid else (fastconformer_tdt_config if tdt else fastconformer_transducer_config)
    cfg = make("small", vocab_size=len(VOCAB), d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16)
    cfg["labels"] = VOCAB
    cfg["decoder"]["prednet"].update(pred_hidden=32, dropout=0.0, pred_rnn_layers=layers)
    cfg["joint"]["jointnet"].update(joint_hidden=32, dropout=0.0)
    cfg["decoding"] = dict(cfg.get("decoding") or {}, **decoding)
    return cfg


def test_models_read_the_beam_section():
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel
    from nemo_amd.modules import BeamBatchedRNNTInfer, BeamBatchedTDTInfer, GreedyBatchedRNNTInfer
    beam = dict(beam_size=8, return_best_hypothesis=False, max_symbols_per_step=3, score_norm=False)
    d = EncDecRNNTModel(_cfg(strategy="malsd_batch", beam=beam)).decoding.decoding
    assert type(d) is BeamBatchedRNNTInfer and (d.beam_size, d.return_best_hypothesis, d.max_symbols) == (8, False, 3)
    d = EncDecRNNTModel(_cfg(tdt=True, strategy="malsd_batch")).decoding.decoding
    assert type(d) is BeamBatchedTDTInfer and (d.beam_size, d.return_best_hypothesis, d.max_symbols) == (4, True, 10) and d.durations
    h = EncDecHybridRNNTCTCModel(_cfg(hybrid=True))
    assert type(h.decoding.decoding) is GreedyBatchedRNNTInfer   # the default strategy is what it was
    h.change_decoding_strategy(dict(strategy="malsd_batch", beam=dict(beam_size=16)), decoder_type="rnnt")
    assert type(h.decoding.decoding) is BeamBatchedRNNTInfer and h.decoding.decoding.beam_size == 16 and h._text_decoding() is h.decoding
    with pytest.raises(NotImplementedError, match="pred_rnn_layers"):
        EncDecRNNTModel(_cfg(layers=2, strategy="malsd_batch")).decoding
    with pytest.raises(NotImplementedError, match="partial_hypotheses.*rnnt_conformer_stream_step"):
        h.decoding.decoding(None, None, partial_hypotheses=[])


@pytest.mark.parametrize("decoding,match", [
    (dict(strategy="malsd_batch", beam=dict(beam_size=17)), "beam_size"),
    (dict(strategy="malsd_batch", beam=dict(score_norm=True)), "score_norm"),
    (dict(strategy="malsd_batch", beam=dict(ngram_lm_model="lm.arpa")), r"beam\.ngram_lm_model"),
    (dict(strategy="malsd_batch", beam=dict(ngram_lm_alpha=0.3)), r"beam\.ngram_lm_alpha"),
    (dict(strategy="malsd_batch", beam=dict(boosting_tree=dict(key_phrases_list=["hey"]))), r"beam\.boosting_tree"),
    (dict(strategy="malsd_batch", beam=dict(allow_cuda_graphs=True)), r"beam\.allow_cuda_graphs"),
    (dict(strategy="malsd_batch", preserve_alignments=True), "preserve_alignments"),
    (dict(strategy="malsd_batch", confidence_cfg=dict(preserve_token_confidence=True)), "confidence_cfg"),
    (dict(strategy="malsd_batch", confidence_cfg=dict(preserve_word_confidence=True)), "confidence_cfg"),
    (dict(strategy="malsd_batch", confidence_cfg=dict(preserve_frame_confidence=True)), "confidence_cfg"),
    (dict(strategy="malsd_batch", greedy=dict(boosting_tree=dict(key_phrases_list=["hey"]), boosting_tree_alpha=1.0)), "boosting_tree"),
    (dict(strategy="beam"), "'beam'"), (dict(strategy="tsd"), "'tsd'"), (dict(strategy="alsd"), "'alsd'"), (dict(strategy="maes"), "'maes'"),
])
def test_what_is_out_of_scope_is_refused_by_name(decoding, match):
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel
    with pytest.raises(NotImplementedError, match=match):
        EncDecRNNTModel(_cfg(**decoding)).decoding
    with pytest.raises(NotImplementedError, match=match):
        h = EncDecHybridRNNTCTCModel(_cfg(hybrid=True))
        h.change_decoding_strategy(decoding, decoder_type="rnnt")
        h.decoding


def _desc(**over):
    """a descriptor the entry would launch (dummy aligned pointers the host never dereferences), with `over` applied"""
    from nemo_amd._lib import TransducerBeamDesc, lib
    p, H, J, V1 = 0x1000, 40, 24, 13
    d = TransducerBeamDesc(enc_proj=p, enc_len=p, emb=p, w_ih=p, w_hh=p, w_pred=p, w_out=p, b_ih=p, b_hh=p, b_pred=p, b_out=p,
                           tokens=p, times=p, out_len=p, score=p, n_hyp=p, workspace=p, ldf=J, ld_ih=H, ld_hh=H, ld_pred=H, ld_out=J,
                           f_dtype=0, w_dtype=0, B=2, T=3, J=J, H=H, V1=V1, blank=V1 - 1, max_symbols=2, max_out=6, beam=4)
    d.workspace_bytes = lib.mi355x_transducer_beam_workspace_bytes(2, 3, H, J, 4, 6)
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("over", [
    dict(beam=0), dict(beam=17), dict(max_out=0), dict(blank=13), dict(V1=1), dict(w_dtype=2), dict(n_hyp=None), dict(workspace=None),
    dict(w_hh=0x1008), dict(ld_hh=42), dict(ld_out=20), dict(workspace_bytes=64), dict(D=3), dict(w_dtype=1, ld_pred=44),
    dict(H=65536, ld_ih=65536, ld_hh=65536, ld_pred=65536, workspace_bytes=1 << 40),   # LDS: three [16, H + 4] float tiles
])
def test_entry_refuses_before_any_launch(over):
    from nemo_amd._lib import lib
    assert _desc().workspace_bytes == 2 * ((2 * 4 * (2 * 40 + 24) * 4 + (1 + 4 * (3 + 6)) * 12 + 15) // 16 * 16)
    assert lib.mi355x_transducer_beam_workspace_bytes(2, 3, 40, 24, 17, 6) == -1
    assert lib.mi355x_transducer_beam_decode(ctypes.byref(_desc(**over)), None) == 1
    assert lib.mi355x_transducer_beam_decode(None, None) == 1
