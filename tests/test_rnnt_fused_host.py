"""CPU: the restatement of the fused greedy transducer search (tests/rnnt_fused_oracle.py) against the unfused restatement and
against itself, the input conditions of the GPU cases (tests/test_rnnt_fused_gpu.py), the `decoding.greedy` keys and their
refusals, the stream state with the model states, and the argument checks of mi355x_transducer_greedy_decode."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ctc_beam_boost_oracle as BO
import ctc_beam_lm_oracle as LO
import rnnt_fused_oracle as R
import stream_decode_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = R.MAX_SYMBOLS
KINDS = ["rnnt", "tdt"]


def _free(case, models, cuts=(), dtype=torch.float64, **kw):
    Pd, Pj = (case["Pd64"], case["Pj64"]) if dtype == torch.float64 else (case["Pd"], case["Pj"])
    return R.decode_chunked_fused(Pd, Pj, case["f_all"].to(dtype), case["lens"], case["V"], MS, list(cuts), models, case["durations"], **kw)


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_without_weights_is_the_unfused_restatement(kind):
    """every alpha = 0, float32 tensors: stream_decode_oracle.decode_chunked's hypotheses and final states"""
    case = R.fused_case(kind)
    models, _ = R.case_models(case, "both", tree_alpha=0.0, lm_alpha=0.0)
    cuts = [5, 14, 27]
    got, fin, _ = _free(case, models, cuts, dtype=torch.float32)
    want, wfin, _ = S.decode_chunked(case["Pd"], case["Pj"], case["enc"], case["lens"], case["V"], MS, cuts, case["durations"],
                                     f_all=case["f_all"])
    assert got == want and sum(len(w[0]) for w in want) > 40
    for a, b in zip(fin, wfin):
        assert torch.equal(a["h"], b["h"]) and torch.equal(a["c"], b["c"])
        assert all(a[k] == b[k] for k in ("last", "frames_done", "skip", "zero_run"))
        assert abs(float(a["score"]) - b["score"]) <= 1e-4 * max(1.0, abs(b["score"]))


@pytest.mark.parametrize("which", ["tree", "lm", "both"])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_chunked_equals_one_shot(kind, which):
    case = R.fused_case(kind)
    models, _ = R.case_models(case, which)
    one, fin1, sc1 = _free(case, models)
    T = S.SMALL["T"]
    for cuts in (list(range(1, T)), [1, 14, 27], [9, 30]):
        got, fin, sc = _free(case, models, cuts)
        assert got == one
        assert all(abs(a - b) <= 1e-9 for a, b in zip(sc, sc1))
        for a, b in zip(fin, fin1):
            assert a["ctx"] == b["ctx"] and a["last"] == b["last"] and a["skip"] == b["skip"] and a["zero_run"] == b["zero_run"]


@pytest.mark.parametrize("which", ["tree", "lm", "both"])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_over_the_tables_equals_the_oracle_over_dict_and_strings(kind, which):
    case = R.fused_case(kind)
    plain, _ = R.case_models(case, which)
    tabled, _ = R.case_models(case, which, tables=True)
    a, _, sa = _free(case, plain)
    b, _, sb = _free(case, tabled)
    assert a == b
    assert all(abs(x - y) <= 1e-9 for x, y in zip(sa, sb)), (sa, sb)


def test_dict_lm_is_cond_logp_over_the_values_the_tables_hold():
    """DictLM.look = the recursion of `cond_logp` with every file value times ln 10 rounded to float32"""
    case = R.fused_case("rnnt")
    lm = R.DictLM(case["ng"], R.LM_ORDER, 1.0)
    g = torch.Generator().manual_seed(5)
    for _ in range(200):
        ctx = tuple(torch.randint(0, case["V"], (int(torch.randint(0, 5, (1,), generator=g)),), generator=g).tolist())
        v = int(torch.randint(0, case["V"], (1,), generator=g))
        want = LO.cond_logp(case["ng"], LO.context_of(ctx, R.LM_ORDER), v)
        assert abs(lm.look(ctx, v) - want) <= 1e-6 * max(1.0, abs(want))


# ---------------------------------------------------------------------------------------------- the inputs of the GPU cases
@pytest.mark.parametrize("which", ["tree", "lm", "both"])
@pytest.mark.parametrize("kind", KINDS)
def test_input_conditions_of_the_small_gpu_cases(kind, which):
    case = R.fused_case(kind)
    models, _ = R.case_models(case, which)
    changed, gaps = [], []
    hyps, fin, _ = _free(case, models, changed=changed, gaps=gaps)
    assert sum(len(h[0]) for h in hyps) > 40
    assert len(changed) >= 10
    for h, base in zip(hyps, case["base"]):
        assert not base[0] or h != base           # the models change every utterance that emits anything
    print(kind, which, "labels", sum(len(h[0]) for h in hyps), "changed", len(changed), "smallest top-2 rank gap", min(gaps))
    if which != "lm":
        tree = models[-1]
        assert any(tree.final(st["ctx"][-1]) < 0 for st in fin)                          # a pending phrase is taken back at the end
        assert any(BO.boost_parts(case["phrases"], h[0])[0] > 0 for h in hyps)           # a hypothesis holds a completed phrase


@pytest.mark.parametrize("kind", KINDS)
def test_input_conditions_of_the_other_gpu_cases(kind):
    # the wide vocabulary
    wide = R.fused_case(kind, "wide")
    assert wide["V"] + 1 > 2 * 512 and (wide["V"] + 1) % 512 != 0
    models, _ = R.case_models(wide, "both")
    changed = []
    hyps, _, _ = R.decode_chunked_fused(wide["Pd64"], wide["Pj64"], wide["f_all"].double(), wide["lens"], wide["V"], MS, [], models,
                                        wide["durations"], changed=changed)
    assert sum(len(h[0]) for h in hyps) > 20 and len(changed) >= 5
    # the chunking case: ragged lengths with a 0; a phrase is pending at the end and the model states moved
    case = R.fused_case(kind)
    for which in ("tree", "both"):
        models, _ = R.case_models(case, which)
        hyps, fin, _ = R.decode_chunked_fused(case["Pd64"], case["Pj64"], case["f_all"].double(), torch.tensor([37, 30, 0, 9]),
                                              case["V"], MS, [], models, case["durations"])
        assert sum(len(h[0]) for h in hyps) > 40 and hyps[2] == ([], [])
        assert any(models[-1].final(st["ctx"][-1]) < 0 for st in fin)


# ---------------------------------------------------------------------------------------------- config
VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


def _ids(text):
    return [VOCAB.index(c) for c in text if c in VOCAB]


def _arpa(tmp_path):
    path = str(tmp_path / "lm.arpa")
    LO.write_arpa(LO.make_lm(0, len(VOCAB), 2), path)
    return path


def test_greedy_section_builds_the_models(tmp_path):
    from nemo_amd.modules import BoostingTree, NGramLM
    from nemo_amd.modules.rnnt_decoding import transducer_fusion_from_config
    f = tmp_path / "phrases.txt"
    f.write_text("bad\n\n  cab  \n", encoding="utf-8")
    greedy = dict(max_symbols=5, ngram_lm_arpa=_arpa(tmp_path), ngram_lm_alpha=0.3, ngram_lm_token_offset=100, boosting_tree_alpha=0.75,
                  boosting_tree=dict(key_phrases_list=["ace"], key_phrases_file=str(f), context_score=2.0, depth_scaling=1.5))
    models = transducer_fusion_from_config(greedy, VOCAB, _ids)
    assert [type(m) for m, _ in models] == [NGramLM, BoostingTree] and [a for _, a in models] == [0.3, 0.75]
    tree = models[1][0]
    assert tree.phrases == ((0, 2, 4), (1, 0, 3), (2, 0, 1)) and (tree.context_score, tree.depth_scaling) == (2.0, 1.5)
    assert models[0][0].vocab_size == tree.vocab_size == len(VOCAB)
    assert transducer_fusion_from_config(greedy, None, None) is None               # the section alone is acceptable
    assert transducer_fusion_from_config(dict(max_symbols=5), VOCAB, _ids) is None   # without the keys nothing changes
    assert transducer_fusion_from_config(None, VOCAB, _ids) is None
    one = transducer_fusion_from_config(dict(boosting_tree=tree, boosting_tree_alpha=1.0), VOCAB, _ids)
    assert one == [(tree, 1.0)]


def test_greedy_section_refusals(tmp_path):
    from nemo_amd.modules.rnnt_decoding import transducer_fusion_from_config as read
    for key in ("ngram_lm_model", "kenlm_path"):
        with pytest.raises(NotImplementedError, match=rf"greedy\.{key}"):
            read({key: "lm.bin"}, VOCAB, _ids)
    with pytest.raises(NotImplementedError, match=r"greedy\.ngram_lm_alpha"):          # a weight without a model
        read(dict(ngram_lm_alpha=0.5), VOCAB, _ids)
    with pytest.raises(ValueError, match=r"greedy\.ngram_lm_alpha"):
        read(dict(ngram_lm_alpha=-0.5, ngram_lm_arpa=_arpa(tmp_path)), VOCAB, _ids)
    with pytest.raises(FileNotFoundError, match=r"greedy\.ngram_lm_arpa"):
        read(dict(ngram_lm_arpa=str(tmp_path / "nowhere.arpa")), VOCAB, _ids)
    with pytest.raises(ValueError, match=r"greedy\.boosting_tree_alpha"):
        read(dict(boosting_tree_alpha=1.0), VOCAB, _ids)
    with pytest.raises(ValueError, match=r"greedy\.boosting_tree_alpha"):
        read(dict(boosting_tree_alpha=-1.0, boosting_tree=dict(key_phrases_list=["ab"])), VOCAB, _ids)
    with pytest.raises(FileNotFoundError, match=r"greedy\.boosting_tree\.key_phrases_file"):
        read(dict(boosting_tree_alpha=1.0, boosting_tree=dict(key_phrases_file=str(tmp_path / "nowhere.txt"))), VOCAB, _ids)
    with pytest.raises(ValueError, match="#%"):                                        # tokenises to nothing
        read(dict(boosting_tree_alpha=1.0, boosting_tree=dict(key_phrases_list=["ab", "#%"])), VOCAB, _ids)
    for key in ("unk_score", "final_eos_score", "score_per_phrase"):
        with pytest.raises(NotImplementedError, match=rf"greedy\.boosting_tree\.{key}"):
            read(dict(boosting_tree_alpha=1.0, boosting_tree={"key_phrases_list": ["ab"], key: 1.0}), VOCAB, _ids)
    # the CTC head's readers keep their own messages
    from nemo_amd.modules import ctc_decoder_from_config
    with pytest.raises(NotImplementedError, match=r"beam\.kenlm_path"):
        ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(kenlm_path="lm.bin")), VOCAB)


def _model_cfg(hybrid, greedy, tdt=False):
    from nemo_amd.models import fastconformer_hybrid_config, fastconformer_tdt_config, fastconformer_transducer_config
    over = dict(d_model=32, n_heads=4, n_layers=1, subsampling_conv_channels=16)
    make = fastconformer_hybrid_config if hybrid else (fastconformer_tdt_config if tdt else fastconformer_transducer_config)
    cfg = make("small", vocab_size=len(VOCAB), **over)
    cfg["labels"] = VOCAB
    cfg["decoder"]["prednet"].update(pred_hidden=32, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=32, dropout=0.0)
    cfg["decoding"] = dict(cfg.get("decoding") or {}, strategy="greedy_batch", greedy=dict(greedy, max_symbols=4))
    return cfg


def test_models_read_the_greedy_section(tmp_path):
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel
    from nemo_amd.modules import BoostingTree, GreedyBatchedTDTInfer, NGramLM
    greedy = dict(boosting_tree=dict(key_phrases_list=["hey there", "it's"]), boosting_tree_alpha=1.5)
    m = EncDecRNNTModel(_model_cfg(False, greedy))
    (tree, alpha), = m.decoding.decoding.fusion_models
    assert isinstance(tree, BoostingTree) and alpha == 1.5 and m.decoding.decoding.max_symbols == 4
    assert tree.phrases == (tuple(_ids("hey there")), tuple(_ids("it's"))) and tree.vocab_size == len(VOCAB)
    m.change_decoding_strategy(dict(strategy="greedy_batch", greedy=dict(max_symbols=4)))
    assert m.decoding.decoding.fusion_models is None
    assert EncDecRNNTModel(_model_cfg(False, {})).decoding.decoding.fusion_models is None
    t = EncDecRNNTModel(_model_cfg(False, dict(greedy, ngram_lm_arpa=_arpa(tmp_path), ngram_lm_alpha=0.2), tdt=True))
    assert isinstance(t.decoding.decoding, GreedyBatchedTDTInfer)
    assert [type(x) for x, _ in t.decoding.decoding.fusion_models] == [NGramLM, BoostingTree]
    h = EncDecHybridRNNTCTCModel(_model_cfg(True, {}))
    assert h.decoding.decoding.fusion_models is None
    h.change_decoding_strategy(dict(strategy="greedy_batch", greedy=greedy), decoder_type="rnnt")
    assert h.decoding.decoding.fusion_models[0][1] == 1.5 and h._text_decoding() is h.decoding
    with pytest.raises(NotImplementedError, match=r"greedy\.kenlm_path"):
        h.change_decoding_strategy(dict(strategy="greedy_batch", greedy=dict(kenlm_path="x")), decoder_type="rnnt")
        h.decoding
    # a confidence asked of the fused search directly is refused too, before anything is projected
    infer = m.decoding.decoding
    assert infer.fusion_models is None
    infer.fusion_models = [(tree, alpha)]
    for call in (infer.decode_ids, infer.decode_ids_stream):
        with pytest.raises(NotImplementedError, match="with_confidence.*fusion_models"):
            call(torch.zeros(1, 32, 3), torch.tensor([3]), with_confidence=True)
    infer.fusion_models = None
    # fusion together with token or word confidence: out of scope, refused by name
    for conf in ({"preserve_token_confidence": True}, {"preserve_word_confidence": True}):
        bad = _model_cfg(False, greedy)
        bad["decoding"]["confidence_cfg"] = conf
        with pytest.raises(NotImplementedError, match="fusion_models.*confidence_cfg"):
            EncDecRNNTModel(bad).decoding


# ---------------------------------------------------------------------------------------------- state, op, ABI
def test_fused_stream_state():
    from nemo_amd import ops
    st = ops.RNNTFusedStreamState.fresh(3, 8, 5, "cpu")
    assert isinstance(st, ops.RNNTStreamState) and len(st.tensors()) == 8
    assert st.m_state.dtype == torch.int32 and st.m_state.tolist() == [[1, 1]] * 3 and st.last.tolist() == [5, 5, 5]
    assert ops.RNNTStreamState.__slots__ == ("h", "c", "last", "score", "frames_done", "skip", "zero_run")
    st.m_state[1] = torch.tensor([4, 7], dtype=torch.int32)
    one = st.select(1)
    assert type(one) is ops.RNNTFusedStreamState and one.m_state.tolist() == [[4, 7]] and one.h.shape == (1, 8)
    back = ops.RNNTFusedStreamState.stack([st.select(2), st.select(1)])
    assert type(back) is ops.RNNTFusedStreamState and back.m_state.tolist() == [[1, 1], [4, 7]] and back.m_state.is_contiguous()
    assert ops.RNNTFusedStreamState.empty(2, 4, "cpu").m_state.shape == (2, 2)
    bad = ops.RNNTFusedStreamState.fresh(2, 4, 3, "cpu")
    bad.m_state = torch.ones(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="m_state"):
        bad._c(2, 4)


def test_op_refuses_wrong_model_lists():
    from nemo_amd import ops
    from nemo_amd.modules import BoostingTree
    tree = BoostingTree.from_phrases([[0, 1]], 4)
    f, lens, emb = torch.zeros(1, 3, 4), torch.tensor([3]), torch.zeros(5, 4)
    w = torch.zeros(16, 4)
    args = (emb, w, 4, w, 4, torch.zeros(16), torch.zeros(16), torch.zeros(4, 4), 4, torch.zeros(4), torch.zeros(5, 4), 4, torch.zeros(5))
    call = lambda models, **kw: ops.transducer_greedy_decode_fused(f, lens, *args, 4, 2, models, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="one or two"):
        call([])
    with pytest.raises(ValueError, match="one or two"):
        call([(tree, 1.0)] * 3)
    with pytest.raises(TypeError):
        call([tree])
    with pytest.raises(TypeError):
        call([(tree.to("cpu"), 1.0)])
    with pytest.raises(ValueError, match="7 labels"):
        call([(BoostingTree.from_phrases([[0]], 7), 1.0)])
    with pytest.raises(TypeError, match="RNNTFusedStreamState"):
        call([(tree, 1.0)], state=ops.RNNTStreamState.fresh(1, 4, 4, "cpu"))


_P = 4096   # non-null: the argument checks return MI_ERR_ARG (1) before anything is launched, the pointers are never followed
_V1 = 9


def _stream_state(**kw):
    from nemo_amd.ops import _StreamStateC
    return _StreamStateC(**dict(dict(h=_P, c=_P + 64, last=_P, score=_P, frames_done=_P, skip=_P, zero_run=_P), **kw))


def _greedy_rc(s_in=None, s_out=None, conf=None, **kw):
    """the return code of mi355x_transducer_greedy_decode for a descriptor that is valid (B=2, T=4, J=H=8, V1=9: the RNN-T one-shot
    search without models) but for the fields given; s_in / s_out = mi355x_rnnt_stream_state, conf = a TransducerConf"""
    from nemo_amd import _lib
    d = _lib.TransducerGreedyDesc(
        enc_proj=_P, f_dtype=0, ldf=8, emb=_P, w_ih=_P, ld_ih=8, w_hh=_P, ld_hh=8, b_ih=_P, b_hh=_P, w_pred=_P, ld_pred=8, b_pred=_P,
        w_out=_P, ld_out=8, b_out=_P, w_dtype=0, B=2, T=4, J=8, H=8, V1=_V1, blank=_V1 - 1, max_symbols=2, tokens=_P, out_len=_P,
        max_out=8)
    for field, obj in (("state_in", s_in), ("state_out", s_out), ("conf", conf)):
        if obj is not None:
            setattr(d, field, C.addressof(obj))
    for k, v in kw.items():
        setattr(d, k, v)
    return _lib.lib.mi355x_transducer_greedy_decode(C.byref(d), None)


def test_fused_entry_is_exported_declared_and_checks_its_arguments():
    from nemo_amd import _lib
    name = "mi355x_transducer_greedy_decode"
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    assert name in set(re.findall(r"\b(mi355x_[a-z0-9_]+)\s*\(", hdr)) and "mi355x_transducer_greedy_desc" in hdr
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(C.CDLL(_lib.LIB_PATH), name)
    from nemo_amd.ops import _CTCBeamFusionC
    p, V1 = _P, _V1
    dur = (C.c_int * 3)(0, 1, 2)

    def model(**kw):
        a = dict(dict(state_arc_begin=p, arc_tok=p, arc_logp=p, arc_next=p, state_bo=p, state_bo_next=p, state_final=None,
                      n_states=4, n_arcs=V1 - 1, alpha=1.0, ub=0.0), **kw)
        return _CTCBeamFusionC(**a)

    def state(m_state=p, **kw):   # a stream state and the automaton states that go with it
        return _stream_state(**kw), m_state

    def rc(models=(model(),), n_models=None, s_in=None, s_out=None, w=p, b=p, dur=None, **kw):
        arr = (_CTCBeamFusionC * max(1, len(models)))(*models) if models is not None else None
        s_in, m_in = s_in or (None, None)
        s_out, m_out = s_out or (None, None)
        return _greedy_rc(s_in, s_out, w_ih=w, w_hh=w, w_pred=w, w_out=w, b_ih=b, b_hh=b, b_pred=b, b_out=b,
                          durations=C.addressof(dur) if dur is not None else None, models=C.addressof(arr) if arr is not None else None,
                          n_models=len(models) if n_models is None and models is not None else (n_models or 0),
                          m_state_in=m_in, m_state_out=m_out, **kw)

    # what the search without models refuses
    for bad in (dict(enc_proj=None), dict(emb=None), dict(w=None), dict(tokens=None), dict(out_len=None), dict(B=0), dict(T=0),
                dict(H=6), dict(J=6), dict(max_out=0), dict(D=3, dur=None), dict(D=1, dur=dur), dict(D=0, dur=dur)):
        assert rc(**bad) == 1, bad
    # the models
    assert rc(models=None, n_models=1) == 1
    assert rc(n_models=0) == 1 and rc(models=(model(),) * 3) == 1
    for tbl in ("state_arc_begin", "arc_tok", "arc_logp", "arc_next", "state_bo", "state_bo_next"):
        assert rc(models=(model(**{tbl: None}),)) == 1, tbl
        assert rc(models=(model(), model(**{tbl: None}))) == 1, tbl
    for bad in (dict(n_states=1), dict(n_arcs=V1 - 2), dict(alpha=-0.5), dict(alpha=float("nan"))):
        assert rc(models=(model(**bad),)) == 1, bad
    assert rc(blank=0) == 1 and rc(blank=V1 - 2) == 1
    # the states
    assert rc(s_out=state(m_state=None)) == 1 and rc(s_in=state(m_state=None), s_out=state(m_state=p + 256, h=p + 128, c=p + 192)) == 1
    assert rc(s_in=state()) == 1                                                       # a state to start from and none to write
    assert rc(s_in=state(), s_out=state()) == 1                                        # aliased
    assert rc(s_in=state(), s_out=state(m_state=p, h=p + 128, c=p + 192)) == 1         # aliased model states
    assert rc(s_in=state(), s_out=state(m_state=p + 256)) == 1                         # aliased h / c
    assert rc(s_out=state(h=None)) == 1 and rc(D=3, dur=dur, s_out=state(skip=None)) == 1


def test_descriptor_entry_refuses_what_no_former_entry_could_be_asked():
    from nemo_amd import _lib
    from nemo_amd.ops import _CTCBeamFusionC
    assert _lib.lib.mi355x_transducer_greedy_decode(None, None) == 1                   # no descriptor
    # a state to start from and none to write, without models
    assert _greedy_rc(s_in=_stream_state()) == 1
    # confidences together with models: the kernel template has no such instantiation
    arr = (_CTCBeamFusionC * 1)(_CTCBeamFusionC(state_arc_begin=_P, arc_tok=_P, arc_logp=_P, arc_next=_P, state_bo=_P, state_bo_next=_P,
                                                state_final=None, n_states=4, n_arcs=_V1 - 1, alpha=1.0, ub=0.0))
    assert _greedy_rc(conf=_lib.TransducerConf(2, 1, 0.33, 1.0, 1.0, 0.0), tok_conf=_P, models=C.addressof(arr), n_models=1) == 1
