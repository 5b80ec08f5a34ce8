"""CPU-side checks of the stateless prediction network, no launch (the pattern of tests/test_rnnt_beam_host.py): the `_target_` builds
the class, widths and keys, refusals by name, the four ABI entries refuse bad arguments, the old configuration builds what it built."""
import ctypes

import pytest

VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


def _cfg(tdt=False, hybrid=False, context=2, **decoding):
    from nemo_amd.models import fastconformer_hybrid_config, fastconformer_tdt_config, fastconformer_transducer_config
    make = fastconformer_hybrid_config if hybrid else (fastconformer_tdt_config if tdt else fastconformer_transducer_config)
    cfg = make("small", vocab_size=len(VOCAB), d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16, stateless_context=context)
    cfg["labels"] = VOCAB
    cfg["decoder"]["prednet"].update(pred_hidden=32, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=32, dropout=0.0)
    cfg["decoding"] = dict(cfg.get("decoding") or {}, **decoding)
    return cfg


def test_the_target_builds_the_class():
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel, fastconformer_transducer_config
    from nemo_amd.modules import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTDecoder, StatelessTransducerDecoder
    m = EncDecRNNTModel(_cfg())
    assert type(m.decoder) is StatelessTransducerDecoder and (m.decoder.context_size, m.decoder.widths) == (2, [24, 8])
    assert (m.decoder.blank_idx, m.decoder.pred_hidden) == (len(VOCAB), 32) and not hasattr(m.decoder, "pred_rnn_layers")
    assert [k for k in m.state_dict() if k.startswith("decoder.")] == [f"decoder.prediction.embeds.{i}.weight" for i in range(2)]
    assert not m.decoder.prediction["embeds"][1].weight[len(VOCAB)].any()   # the padding row
    assert type(m.decoding.decoding) is GreedyBatchedRNNTInfer and m.decoding.decoding.stateless
    assert type(EncDecRNNTModel(_cfg(tdt=True)).decoding.decoding) is GreedyBatchedTDTInfer
    assert type(EncDecHybridRNNTCTCModel(_cfg(hybrid=True)).decoder) is StatelessTransducerDecoder
    for E, C, want in [(200, 2, [150, 50]), (40, 3, [28, 6, 6]), (32, 1, [32])]:   # slice widths
        dec = StatelessTransducerDecoder(prednet=dict(pred_hidden=E, dropout=0.1), vocab_size=10, context_size=C)
        assert dec.widths == want and [tuple(e.weight.shape) for e in dec.prediction["embeds"]] == [(11, w) for w in want]
    # without the new key: exactly what it was
    assert fastconformer_transducer_config("small") == fastconformer_transducer_config("small", stateless_context=None)
    old = EncDecRNNTModel(_cfg(context=None))
    assert type(old.decoder) is RNNTDecoder and not old.decoding.decoding.stateless and "_target_" not in _cfg(context=None)["decoder"]


@pytest.mark.parametrize("kw,decoding,match", [
    (dict(normalization_mode="layer"), {}, "normalization_mode"), (dict(context_size=5), {}, "context_size"),
    (dict(random_state_sampling=True), {}, "random_state_sampling"),
    ({}, dict(strategy="malsd_batch"), "malsd_batch.*StatelessTransducerDecoder"),
    ({}, dict(confidence_cfg=dict(preserve_token_confidence=True)), "confidence_cfg.*StatelessTransducerDecoder"),
    ({}, dict(confidence_cfg=dict(preserve_word_confidence=True)), "confidence_cfg.*StatelessTransducerDecoder"),
    ({}, dict(confidence_cfg=dict(preserve_frame_confidence=True)), "frame confidences"),
    ({}, dict(greedy=dict(boosting_tree=dict(key_phrases_list=["hey"]), boosting_tree_alpha=1.0)), "fusion_models.*StatelessTransducerDecoder"),
])
def test_what_is_out_of_scope_is_refused_by_name(kw, decoding, match):
    from nemo_amd.models import EncDecRNNTModel
    for tdt in (False, True):
        cfg = _cfg(tdt=tdt, **decoding)
        cfg["decoder"].update(kw)
        with pytest.raises(NotImplementedError, match=match):
            EncDecRNNTModel(cfg).decoding


def _desc(**over):   # a descriptor the entry would launch (dummy aligned pointers the host never dereferences), with `over` applied
    from nemo_amd._lib import StatelessGreedyDesc
    p, J, V1 = 0x1000, 24, 13
    d = StatelessGreedyDesc(enc_proj=p, enc_len=p, tables=p, b_pred=p, w_out=p, b_out=p, tokens=p, times=p, out_len=p, score=p, ldf=J,
                            ld_out=J, f_dtype=0, w_dtype=0, B=2, T=3, J=J, V1=V1, C=2, blank=V1 - 1, max_symbols=2, max_out=6)
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("over", [
    dict(C=0), dict(C=5), dict(blank=13), dict(blank=-1), dict(V1=1), dict(max_out=0), dict(T=0), dict(w_dtype=2), dict(f_dtype=2),
    dict(tables=None), dict(b_pred=None), dict(tokens=None), dict(w_out=0x1008), dict(ld_out=20), dict(ld_out=26), dict(ldf=22),
    dict(w_dtype=1, J=20, ld_out=24), dict(D=3), dict(J=65536, ld_out=65536, ldf=65536),   # LDS: the [16, J + 4] float tile
])
def test_greedy_entry_refuses_before_any_launch(over):
    from nemo_amd._lib import lib
    from nemo_amd.ops import _StatelessStateC
    assert lib.mi355x_stateless_greedy_decode(ctypes.byref(_desc(**over)), None) == 1
    assert lib.mi355x_stateless_greedy_decode(None, None) == 1
    st, part = _StatelessStateC(*(0x2000 + 64 * i for i in range(5))), _StatelessStateC(*(0x2000 + 64 * i for i in range(4)))
    for states in (dict(state_in=ctypes.addressof(st)), dict(state_out=ctypes.addressof(part)),
                   dict(state_in=ctypes.addressof(st), state_out=ctypes.addressof(st))):   # in without out; not whole; aliased
        assert lib.mi355x_stateless_greedy_decode(ctypes.byref(_desc(**states)), None) == 1


def test_training_and_table_entries_refuse_before_any_launch():
    from nemo_amd._lib import lib
    p = 0x1000
    tabs, hole = (ctypes.c_void_p * 2)(p, p), (ctypes.c_void_p * 2)(p, None)
    call = lambda fn, names, base, k, tail=(0, 0, 1.0, None): fn(*[{**base, **k}[n] for n in names.split()], *tail)   # (tail: no dropout)
    dims = dict(dt=0, B=2, U=3, E=32, C=2, V1=13, bl=12)
    fwd = lambda **k: call(lib.mi355x_stateless_pred_fwd, "t e o dt B U E C V1 bl", dict(dims, t=p, e=tabs, o=p), k)
    bwd = lambda **k: call(lib.mi355x_stateless_embed_bwd, "t g dt e a B U E C V1 bl", dict(dims, t=p, g=p, e=tabs, a=0), k)
    tab = lambda **k: call(lib.mi355x_stateless_tables, "e w ld dt o E C V1 J bl", dict(dims, e=tabs, w=p, ld=32, o=p, J=24), k, (None,))
    for bad in (dict(C=0), dict(C=5), dict(bl=13), dict(V1=1), dict(dt=2), dict(e=hole), dict(e=None), dict(E=2, C=4)):
        assert fwd(**bad) == 1 and bwd(**bad) == 1 and tab(**bad) == 1, bad
    assert fwd(t=None) == 1 and fwd(o=0x1004) == 1 and fwd(B=0) == 1 and fwd(U=-1) == 1 and fwd(B=1 << 20, U=1 << 10) == 1
    assert bwd(g=None) == 1 and bwd(g=0x1004) == 1 and bwd(B=0) == 1
    assert tab(w=None) == 1 and tab(o=None) == 1 and tab(ld=31) == 1 and tab(J=0) == 1 and tab(o=0x1004) == 1
