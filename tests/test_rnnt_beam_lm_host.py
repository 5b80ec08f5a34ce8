"""CPU-side checks of the fused transducer beam search (no kernel is launched): the entry is declared, exported and refuses bad
arguments before any launch; `beam.ngram_lm_arpa` is read by the transducer model and the hybrid model's transducer head; what
stays out of scope is refused by name."""
import ctypes
import os

import pytest

import ctc_beam_lm_oracle as L
from test_rnnt_beam_host import VOCAB, _cfg, _desc


def _arpa(tmp_path):
    L.write_arpa(L.make_lm(0, len(VOCAB), 3), tmp_path / "lm.arpa")
    return str(tmp_path / "lm.arpa")


def _fusion(n=1, **over):
    from nemo_amd.ops import _CTCBeamFusionC
    arr = (_CTCBeamFusionC * max(n, 1))()
    for i in range(max(n, 1)):
        arr[i] = _CTCBeamFusionC(*([0x1000] * 6), None, 5, 40, 0.5, 0.0)
        for k, v in over.items():
            setattr(arr[i], k, v)
    return arr


@pytest.mark.parametrize("n,over", [(0, {}), (2, {}), (1, dict(state_final=0x1000)), (1, dict(arc_next=None)), (1, dict(n_states=1)),
                                    (1, dict(n_arcs=11)), (1, dict(alpha=-0.5)), (1, dict(alpha=float("nan"))),
                                    (1, dict(alpha=float("inf")))])
def test_entry_is_exported_and_refuses_before_any_launch(n, over):
    from nemo_amd import _lib
    assert "mi355x_transducer_beam_decode_fused" in _lib.EXPORTED_SYMBOLS
    assert "int mi355x_transducer_beam_decode_fused(" in open(os.path.join(os.path.dirname(__file__), "..", "include", "mi355x_asr.h")).read()
    fn = _lib.lib.mi355x_transducer_beam_decode_fused
    assert fn(None, ctypes.addressof(_fusion()), 1, None) == 1
    assert fn(ctypes.byref(_desc()), None, 1, None) == 1
    assert fn(ctypes.byref(_desc(beam=17)), ctypes.addressof(_fusion()), 1, None) == 1   # (what the plain entry refuses)
    assert fn(ctypes.byref(_desc(blank=3)), ctypes.addressof(_fusion()), 1, None) == 1   # (the blank is the last class)
    assert fn(ctypes.byref(_desc()), ctypes.addressof(_fusion(n, **over)), n, None) == 1


@pytest.mark.parametrize("hybrid", [False, True])
def test_models_read_the_beam_sections_model(hybrid, tmp_path):
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel
    from nemo_amd.modules import BeamBatchedRNNTInfer, NGramLM
    dec = dict(strategy="malsd_batch", beam=dict(beam_size=4, ngram_lm_arpa=_arpa(tmp_path), ngram_lm_alpha=0.5, ngram_lm_token_offset=100,
                                                 blank_lm_score_mode="no_score", pruning_mode="late"))
    if hybrid:
        m = EncDecHybridRNNTCTCModel(_cfg(hybrid=True))
        m.change_decoding_strategy(dec, decoder_type="rnnt")
    else:
        m = EncDecRNNTModel(_cfg(**dec))
    d = m.decoding.decoding
    (lm, alpha), = d.fusion_models
    assert type(d) is BeamBatchedRNNTInfer and isinstance(lm, NGramLM) and lm.vocab_size == len(VOCAB) and alpha == 0.5 and lm.order == 3
    m.change_decoding_strategy(dict(strategy="malsd_batch"), **(dict(decoder_type="rnnt") if hybrid else {}))
    assert m.decoding.decoding.fusion_models is None   # without the keys the search is the plain one


def test_what_stays_out_of_scope_is_refused_by_name(tmp_path):
    from nemo_amd.models import EncDecRNNTModel
    from nemo_amd.modules import BeamBatchedRNNTInfer
    from nemo_amd.modules.boosting_tree import BoostingTree
    from nemo_amd.modules.rnnt_decoding import transducer_beam_from_config as read
    arpa = _arpa(tmp_path)
    model = EncDecRNNTModel(_cfg())
    tree = BoostingTree.from_phrases([[1, 2]], len(VOCAB))
    with pytest.raises(NotImplementedError, match="BoostingTree"):
        BeamBatchedRNNTInfer(model.decoder, model.joint, len(VOCAB), fusion_models=[(tree, 1.0)])
    for key, ok, bad in (("blank_lm_score_mode", "no_score", "lm_weighted_full"), ("pruning_mode", "late", "early")):
        read(dict(strategy="malsd_batch", beam={"ngram_lm_arpa": arpa, key: ok}))
        with pytest.raises(NotImplementedError, match=rf"beam\.{key}"):
            read(dict(strategy="malsd_batch", beam={"ngram_lm_arpa": arpa, key: bad}))
    with pytest.raises(ValueError, match=r"beam\.ngram_lm_alpha"):
        read(dict(strategy="malsd_batch", beam=dict(ngram_lm_arpa=arpa, ngram_lm_alpha=-1.0)))
    with pytest.raises(FileNotFoundError, match=r"beam\.ngram_lm_arpa"):
        read(dict(strategy="malsd_batch", beam=dict(ngram_lm_arpa=str(tmp_path / "nowhere.arpa"))))
    with pytest.raises(NotImplementedError, match=r"beam\.ngram_lm_model"):
        read(dict(strategy="malsd_batch", beam=dict(ngram_lm_arpa=arpa, ngram_lm_model="lm.bin")))
