"""CPU-side checks of the multi-blank transducer, no launch: the configuration builds the loss and decoder classes and the joint
width, refusals by name, the loss entry refuses bad arguments before any launch, the TDT and RNN-T configurations build what they built."""
import ctypes

import pytest

VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


def _cfg(make="multiblank", **decoding):
    from nemo_amd import models
    cfg = getattr(models, f"fastconformer_{make}_config")("small", vocab_size=len(VOCAB), d_model=32, n_heads=4, n_layers=1,
                                                         subsampling_conv_channels=16)
    cfg["labels"] = VOCAB
    cfg["decoder"]["prednet"].update(pred_hidden=32, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=32, dropout=0.0)
    cfg["decoding"] = dict(cfg.get("decoding") or {}, **decoding)
    return cfg


def test_the_configuration_builds_the_classes():
    from nemo_amd.models import EncDecRNNTModel
    from nemo_amd.modules import (GreedyBatchedMultiblankRNNTInfer, GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, MultiblankRNNTLoss,
                                  MultiblankRNNTLossNumba, RNNTLoss, TDTLoss)
    m = EncDecRNNTModel(_cfg())
    V = len(VOCAB)
    assert type(m.loss) is MultiblankRNNTLoss is MultiblankRNNTLossNumba and (m.loss.blank, m.loss.big_blank_durations) == (V + 3, [2, 4, 8])
    assert m.loss.sigma == 0.05 and m.joint.joint_net[-1].weight.shape[0] == V + 1 + 3 and m.decoder.blank_idx == V
    assert tuple(m.decoder.prediction["embed"].weight.shape) == (V + 1, 32)   # the prediction network is the RNN-T one
    dec = m.decoding.decoding
    assert type(dec) is GreedyBatchedMultiblankRNNTInfer and (dec._blank_index, dec.big_blank_durations) == (V, [2, 4, 8])
    assert m.decoding.ids_to_text([0, 1, V]) == "ab"
    for make, loss, infer, width in (("transducer", RNNTLoss, GreedyBatchedRNNTInfer, V + 1), ("tdt", TDTLoss, GreedyBatchedTDTInfer, V + 6)):
        old = EncDecRNNTModel(_cfg(make))
        assert type(old.loss) is loss and type(old.decoding.decoding) is infer and old.joint.joint_net[-1].weight.shape[0] == width


@pytest.mark.parametrize("decoding,decoder,match", [
    (dict(strategy="malsd_batch"), {}, "malsd_batch.*multi-blank"),
    (dict(greedy=dict(boosting_tree=dict(key_phrases_list=["hey"]), boosting_tree_alpha=1.0)), {}, "multi-blank.*fusion models"),
    (dict(confidence_cfg=dict(preserve_token_confidence=True)), {}, "multi-blank.*confidence_cfg"),
    ({}, dict(prednet=dict(pred_hidden=32, pred_rnn_layers=2, dropout=0.0)), "multiblank_rnnt.*pred_rnn_layers"),
    ({}, dict(_target_="nemo.collections.asr.modules.StatelessTransducerDecoder", context_size=2), "multiblank_rnnt.*Stateless"),
])
def test_what_is_out_of_scope_is_refused_by_name(decoding, decoder, match):
    from nemo_amd.models import EncDecRNNTModel
    cfg = _cfg(**decoding)
    cfg["decoder"].update(decoder)
    with pytest.raises(NotImplementedError, match=match):
        EncDecRNNTModel(cfg).decoding


def test_loss_knobs_alignment_and_the_hybrid_model_are_refused_by_name():
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel, fastconformer_hybrid_config
    from nemo_amd.modules import MultiblankRNNTLoss
    for kw, match in ((dict(fastemit_lambda=0.01), "fastemit_lambda"), (dict(clamp=1.0), "clamp")):
        with pytest.raises(NotImplementedError, match=match):
            MultiblankRNNTLoss(blank=31, big_blank_durations=[2, 4], **kw)
    m = EncDecRNNTModel(_cfg())
    with pytest.raises(NotImplementedError, match="align.*multi-blank"):
        m.align(["x.wav"], ["a"])
    hyb = fastconformer_hybrid_config("small", vocab_size=len(VOCAB), d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16)
    hyb["labels"], hyb["loss"] = VOCAB, _cfg()["loss"]
    with pytest.raises(NotImplementedError, match="multiblank_rnnt.*hybrid"):
        EncDecHybridRNNTCTCModel(hyb)


def test_the_c_entries_refuse_before_any_launch():   # (dummy aligned pointers; each call is `over` away from one that would launch)
    from nemo_amd._lib import TransducerConf, TransducerGreedyDesc, lib
    from nemo_amd.ops import _StreamStateC
    p, ints = 0x1000, lambda v: (ctypes.c_int * max(len(v), 1))(*v)
    for over in (dict(nb=0, dur=[2]), dict(nb=8, dur=list(range(2, 10))), dict(nb=1, dur=[1]), dict(nb=1, dur=[9]), dict(dur=[4, 2, 8]),
                 dict(dur=[2, 2, 8]), dict(blank=10), dict(blank=12), dict(sigma=-0.1), dict(sigma=float("nan")), dict(U1=1025), dict(ld=11),
                 dict(ldg=11), dict(gdt=1, ldg=12), dict(ws=10), dict(N=4), dict(B=0)):
        a = dict(dict(ld=12, B=2, T=5, U1=3, N=12, nb=3, dur=[2, 4, 8], blank=11, sigma=0.0, ldg=12, gdt=0), **over)
        a.setdefault("ws", (5 + a["nb"]) * a["B"] * a["T"] * a["U1"] + 2 * a["B"])
        assert lib.mi355x_multiblank_loss_ex(p, a["ld"], p, p, p, a["B"], a["T"], a["U1"], a["N"], a["nb"], ints(a["dur"]), a["blank"],
                                             a["sigma"], 1.0, p, p, a["gdt"], a["ldg"], p, a["ws"], None) == 1, over
    tdt, conf = ints([0, 1, 2]), TransducerConf(0, 0, 1.0, 0.0, 0.0, 0.0)
    part = _StreamStateC(*(0x2000 + 64 * i for i in range(5)))   # a state without skip / zero_run
    kw = dict(enc_proj=p, enc_len=p, emb=p, w_ih=p, w_hh=p, w_pred=p, w_out=p, b_ih=p, b_hh=p, b_pred=p, b_out=p, tokens=p, times=p,
              out_len=p, score=p, ldf=8, ld_ih=8, ld_hh=8, ld_pred=8, ld_out=8, f_dtype=0, w_dtype=0, B=2, T=3, J=8, H=8, V1=10, blank=9,
              max_symbols=2, max_out=6)
    search = lambda dur, **over: lib.mi355x_transducer_greedy_decode_multiblank(ctypes.byref(TransducerGreedyDesc(**dict(kw, **over))),
                                                                                len(dur), ints(dur), None)
    for over in (dict(D=3, durations=ctypes.addressof(tdt)), dict(conf=ctypes.addressof(conf), tok_conf=p), dict(models=p, n_models=1),
                 dict(blank=8), dict(state_out=ctypes.addressof(part)), dict(tokens=None)):
        assert search([2, 4, 8], **over) == 1, over
    for dur in ([], [1, 4, 8], [2, 4, 9], [4, 2, 8], list(range(2, 10))):
        assert search(dur) == 1, dur
