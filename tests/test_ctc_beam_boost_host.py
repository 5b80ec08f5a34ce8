"""No GPU: phrase boosting of the CTC beam search.  `BoostingTree` (the Aho-Corasick automaton flattened into the kernel's tables)
against the brute-force definition of tests/ctc_beam_boost_oracle.py (string matching, no trie), its tables against `NGramLM._check`
and its bound against an exhaustive search; the refusals; config parsing; the fused entries' C ABI (header, ctypes list, struct
mirrors, the argument checks that come before any launch); `CTCBeamStreamState` with the second model's storage."""
import ctypes
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import ctc_beam_boost_oracle as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355x_ctc_beam_decode_fused", "mi355x_ctc_beam_decode_fused_stream")
STATE_FIELDS = ("node", "par", "tok", "len", "h", "hp", "pb", "pnb", "tot", "brank", "lm_state", "lm_sum", "nb", "frames_done")
FUSION_FIELDS = ("state_arc_begin", "arc_tok", "arc_logp", "arc_next", "state_bo", "state_bo_next", "state_final", "n_states", "n_arcs",
                 "alpha", "ub")


def _tree(phrases, V, cs=1.0, ds=2.0):
    from nemo_amd.modules import BoostingTree
    return BoostingTree.from_phrases(phrases, V, context_score=cs, depth_scaling=ds)


def _same(tree, phrases, y, cs, ds):
    complete, pending = B.boost_parts(phrases, y, cs, ds)
    boost, final = tree.score(y)
    assert abs(boost - (complete + pending)) <= 1e-9 and abs(final - complete) <= 1e-9, (phrases, y, boost, final, complete, pending)
    return complete, pending


# ---------------------------------------------------------------------------------------------- the table walk against brute force
def test_hand_cases():
    # nested: `new` / `new york` (ids 0, 1); cs = 1, ds = 2: ts = 1, 2; full(new) = 1, full(new york) = 3
    ph = [(0,), (0, 1)]
    t = _tree(ph, 4)
    assert _same(t, ph, (0,), 1, 2) == (1.0, 1.0)
    assert _same(t, ph, (0, 1), 1, 2) == (4.0, 3.0)        # both completed; the whole phrase is still a pending prefix
    assert _same(t, ph, (0, 1, 2), 1, 2) == (4.0, 0.0)
    assert _same(t, ph, (0, 2), 1, 2) == (1.0, 0.0)
    # overlapping: `a b` / `b c d`
    ph = [(0, 1), (1, 2, 3)]
    t = _tree(ph, 5)
    assert _same(t, ph, (0, 1), 1, 2) == (3.0, 3.0)
    assert _same(t, ph, (0, 1, 2), 1, 2) == (3.0, 3.0)     # a b completed, b c pending: the failure link kept the b
    assert _same(t, ph, (0, 1, 2, 3), 1, 2) == (8.0, 5.0)
    assert _same(t, ph, (0, 1, 2, 4), 1, 2) == (3.0, 0.0)
    # a phrase occurring twice, and overlapping itself
    ph = [(2, 2)]
    t = _tree(ph, 3)
    assert _same(t, ph, (2, 2, 0, 2, 2), 1, 2) == (6.0, 3.0)
    assert _same(t, ph, (2, 2, 2), 1, 2) == (6.0, 3.0)     # two end positions
    # a failing sibling: `a b c` begun, `a b a ...` taken back to the suffix `a`, which begins the phrase again
    ph = [(0, 1, 2)]
    t = _tree(ph, 3)
    assert _same(t, ph, (0, 1), 1, 2) == (0.0, 3.0)
    assert _same(t, ph, (0, 1, 0), 1, 2) == (0.0, 1.0)
    assert _same(t, ph, (0, 1, 1), 1, 2) == (0.0, 0.0)
    # a suffix of the failed match is a prefix of ANOTHER phrase: `a b c` / `b d`
    ph = [(0, 1, 2), (1, 3)]
    t = _tree(ph, 4)
    assert _same(t, ph, (0, 1), 1, 2) == (0.0, 3.0)
    assert _same(t, ph, (0, 1, 3), 1, 2) == (3.0, 3.0)
    # other scores (float32 values: the tables hold float32, and `score` walks those tables); duplicates are one phrase
    ph = [(1, 2, 3), (1, 2, 3), (3,)]
    t = _tree(ph, 4, cs=0.75, ds=1.5)
    assert len(t.phrases) == 2
    _same(t, ph, (1, 2, 3, 3, 1, 2), 0.75, 1.5)


def test_random_sequences_match_brute_force():
    rng = np.random.default_rng(5)
    for trial in range(120):
        V = int(rng.integers(2, 7))
        ph = [tuple(rng.integers(0, V, size=int(rng.integers(1, 5))).tolist()) for _ in range(int(rng.integers(1, 9)))]
        cs, ds = float(rng.choice([1.0, 2.0, 0.75])), float(rng.choice([1.0, 2.0, 1.5]))
        t = _tree(ph, V, cs, ds)
        bt = B._Boost(ph, V, cs, ds)
        for _ in range(12):
            y = tuple(rng.integers(0, V, size=int(rng.integers(0, 14))).tolist())
            complete, pending = _same(t, ph, y, cs, ds)
            assert abs(sum(bt.of(y)) - (complete + pending)) <= 1e-9       # (the oracle's cached form is the definition too)
            if y:
                assert abs(bt.row(y[:-1])[y[-1]] - (complete + pending)) <= 1e-9


def test_generated_phrase_sets_match_brute_force():
    """the phrase sets of the GPU test's shapes, on the arg-max paths they come from"""
    import ctc_beam_oracle as O
    for T, C, cs, ds in ((37, 5, 1.0, 2.0), (24, 129, 1.0, 2.0), (66, 129, 2.0, 1.0)):
        ph = B.make_phrases(T, C)
        assert 40 <= len(ph) <= 120 and len(set(ph)) == len(ph)
        t = _tree(ph, C - 1, cs, ds)
        for seed in range(4):
            y = tuple(B.collapse(O.make_logp(seed, T, C).argmax(axis=1).tolist(), C - 1))
            complete, _ = _same(t, ph, y, cs, ds)
            assert complete > 0


# ---------------------------------------------------------------------------------------------- tables and bound
def test_tables_pass_the_ngram_checks_and_have_the_stated_form():
    from nemo_amd.modules import NGramLM
    ph = [(0, 1, 2), (1, 3), (0,), (4, 4)]
    t = _tree(ph, 6)
    assert isinstance(t, NGramLM)
    t._check()
    S, V = t.num_states, 6
    assert t.state_arc_begin[1] == V and t.state_arc_begin[2] == V                      # state 1: no arcs
    assert t.state_bo[1] == 0 and t.state_bo_next[1] == 0 and t.state_final[0] == 0 and t.state_final[1] == 0
    assert t.state_final.shape == (S,) and t.state_final.dtype == np.float32 and (t.state_final[2:] < 0).all()
    assert (t.arc_logp[:V][[2, 3, 5]] == 0).all() and (t.arc_next[:V][[2, 3, 5]] == 0).all()   # labels that start no phrase
    assert (t.state_bo <= 0).all() and (t.arc_logp >= 0).all()
    tabs = t.to("cpu")
    assert len(tabs) == 7 and tabs[6].dtype == torch.float32 and tabs[0].dtype == torch.int32
    assert t.to("cpu") is tabs
    assert np.array_equal(tabs[6].numpy(), t.state_final)


def test_upper_bound_covers_every_lookup():
    ph = [(0, 1, 2), (1, 2), (2,), (1, 2, 0, 1), (3, 3)]
    t = _tree(ph, 4, cs=1.5, ds=2.0)
    worst = max(t.lookup(s, c)[0] for s in range(t.num_states) for c in range(4))
    assert worst > 0 and t.lm_ub >= worst
    # and over the states sequences actually reach, by exhaustion to length 5
    for y in itertools.product(range(4), repeat=5):
        s = 1
        for c in y:
            v, s = t.lookup(s, c)
            assert v <= t.lm_ub


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_phrase():
    from nemo_amd.modules import BoostingTree
    with pytest.raises(ValueError, match="empty"):
        BoostingTree.from_phrases([], 4)
    with pytest.raises(ValueError, match="phrase 1 is empty"):
        BoostingTree.from_phrases([[0], []], 4)
    with pytest.raises(ValueError, match=r"phrase 2 = \[1, 4\]"):
        BoostingTree.from_phrases([[0], [1], [1, 4]], 4)
    with pytest.raises(ValueError, match=r"phrase 0 = \[-1\]"):
        BoostingTree.from_phrases([[-1]], 4)
    for kw in (dict(context_score=0.0), dict(depth_scaling=-1.0), dict(context_score=float("nan"))):
        with pytest.raises(ValueError):
            BoostingTree.from_phrases([[0]], 4, **kw)


def test_decoder_refusals():
    from nemo_amd.modules import BeamBatchedCTCDecoder, NGramLM
    t = _tree([(0, 1)], 3)
    d = BeamBatchedCTCDecoder(list("abc"), boosting_tree=t, boosting_tree_alpha=0.5)
    assert d.boosting_tree is t and d.boosting_tree_alpha == 0.5 and d._fusion_models() == [(t, 0.5)]
    with pytest.raises(ValueError):
        BeamBatchedCTCDecoder(list("abc"), boosting_tree=t, boosting_tree_alpha=-1.0)
    with pytest.raises(ValueError):
        BeamBatchedCTCDecoder(list("abcd"), boosting_tree=t)
    with pytest.raises(TypeError):
        BeamBatchedCTCDecoder(list("abc"), boosting_tree=t.to("cpu"))
    plain = BeamBatchedCTCDecoder(list("abc"))
    assert plain.boosting_tree is None and plain.boosting_tree_alpha == 0.0


def test_ops_refuse_loose_tensors_and_wrong_lists():
    from nemo_amd import ops
    t = _tree([(0, 1)], 4)
    logp = torch.zeros(1, 3, 5)
    for f, extra in ((ops.ctc_beam_decode_fused, ()), (ops.ctc_beam_decode_fused_stream, (None,))):
        with pytest.raises(TypeError):
            f(logp, None, 4, 4, 20.0, 0.0, *extra, [(t.to("cpu"), 1.0)])
        with pytest.raises(TypeError):
            f(logp, None, 4, 4, 20.0, 0.0, *extra, [t])
        with pytest.raises(ValueError):
            f(logp, None, 4, 4, 20.0, 0.0, *extra, [])
        with pytest.raises(ValueError):
            f(logp, None, 4, 4, 20.0, 0.0, *extra, [(t, 1.0)] * 3)
        with pytest.raises(ValueError):
            f(logp, None, 4, 4, 20.0, 0.0, *extra, [(_tree([(0,)], 7), 1.0)])


# ---------------------------------------------------------------------------------------------- config
def _ids(text):
    return [ord(c) - ord("a") for c in text if "a" <= c <= "e"]


def test_config_builds_the_tree(tmp_path):
    from nemo_amd.modules import BeamBatchedCTCDecoder, BoostingTree, ctc_decoder_from_config
    vocab = list("abcde")
    f = tmp_path / "phrases.txt"
    f.write_text("bad\n\n  cab  \n", encoding="utf-8")
    cfg = {"strategy": "beam_batch", "beam": {"beam_size": 8, "boosting_tree_alpha": 0.75,
                                              "boosting_tree": {"key_phrases_list": ["ace", "bad"], "key_phrases_file": str(f),
                                                                "context_score": 2.0, "depth_scaling": 1.5}}}
    d = ctc_decoder_from_config(cfg, vocab, text_to_ids=_ids)
    assert type(d) is BeamBatchedCTCDecoder and isinstance(d.boosting_tree, BoostingTree) and d.boosting_tree_alpha == 0.75
    assert d.boosting_tree.phrases == ((0, 2, 4), (1, 0, 3), (2, 0, 1)) and d.boosting_tree.vocab_size == 5
    assert (d.boosting_tree.context_score, d.boosting_tree.depth_scaling) == (2.0, 1.5) and d.ngram_lm is None
    assert ctc_decoder_from_config(cfg, None) is None                              # the section alone is acceptable
    # a ready tree; no tree: the decoder of before
    t = _tree([(0, 1)], 5)
    d = ctc_decoder_from_config({"strategy": "beam_batch", "beam": {"boosting_tree": t, "boosting_tree_alpha": 1.0}}, vocab)
    assert d.boosting_tree is t
    d = ctc_decoder_from_config({"strategy": "beam_batch", "beam": {"beam_size": 8}}, vocab)
    assert d.boosting_tree is None and d.boosting_tree_alpha == 0.0
    # the defaults of the three reference keys pass
    ok = {"strategy": "beam_batch", "beam": {"boosting_tree_alpha": 1.0, "boosting_tree": {
        "key_phrases_list": ["ab"], "unk_score": 0.0, "final_eos_score": 0.0, "score_per_phrase": 0.0}}}
    assert ctc_decoder_from_config(ok, vocab, text_to_ids=_ids).boosting_tree.phrases == ((0, 1),)


def test_config_refusals(tmp_path):
    from nemo_amd.modules import ctc_decoder_from_config
    vocab = list("abcde")
    beam = lambda **kw: {"strategy": "beam_batch", "beam": kw}
    for key in ("unk_score", "final_eos_score", "score_per_phrase"):
        with pytest.raises(NotImplementedError, match=key):
            ctc_decoder_from_config(beam(boosting_tree_alpha=1.0, boosting_tree={"key_phrases_list": ["ab"], key: 1.0}), vocab,
                                    text_to_ids=_ids)
    with pytest.raises(ValueError, match="xyz"):                                     # tokenises to nothing
        ctc_decoder_from_config(beam(boosting_tree_alpha=1.0, boosting_tree={"key_phrases_list": ["ab", "xyz"]}), vocab, text_to_ids=_ids)
    with pytest.raises(ValueError, match="boosting_tree_alpha"):                     # a weight without phrases
        ctc_decoder_from_config(beam(boosting_tree_alpha=1.0), vocab, text_to_ids=_ids)
    with pytest.raises(ValueError, match="boosting_tree_alpha"):
        ctc_decoder_from_config(beam(boosting_tree_alpha=-1.0, boosting_tree={"key_phrases_list": ["ab"]}), vocab, text_to_ids=_ids)
    missing = str(tmp_path / "nowhere.txt")
    with pytest.raises(FileNotFoundError):
        ctc_decoder_from_config(beam(boosting_tree_alpha=1.0, boosting_tree={"key_phrases_file": missing}), vocab, text_to_ids=_ids)
    with pytest.raises(FileNotFoundError):                                           # also where the section is only checked
        ctc_decoder_from_config(beam(boosting_tree_alpha=1.0, boosting_tree={"key_phrases_file": missing}), None)


def test_hybrid_keeps_its_decoding_when_the_file_is_missing(tmp_path):
    """change_decoding_strategy checks the section before it replaces anything"""
    from nemo_amd.models import hybrid_models
    with pytest.raises(FileNotFoundError):
        hybrid_models._check_ctc_strategy({"strategy": "beam_batch", "beam": {"boosting_tree_alpha": 1.0, "boosting_tree": {
            "key_phrases_file": str(tmp_path / "nowhere.txt")}}})


# ---------------------------------------------------------------------------------------------- C ABI
def test_symbols_and_structs_are_declared_and_listed():
    from nemo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    declared = set(re.findall(r"\b(mi355x_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct mi355x_ctc_beam_fusion \{.*?state_final.*?\} mi355x_ctc_beam_fusion;", hdr, re.S)
    assert re.search(r"typedef struct mi355x_ctc_beam_fused_state \{.*?fs_state.*?fs_sum.*?\} mi355x_ctc_beam_fused_state;", hdr, re.S)


def test_struct_mirrors_match_the_header():
    from nemo_amd.ops import _CTCBeamFusedStateC, _CTCBeamFusionC, _CTCBeamStateC
    assert tuple(n for n, _ in _CTCBeamFusionC._fields_) == FUSION_FIELDS
    assert tuple(n for n, _ in _CTCBeamFusedStateC._fields_) == ("beams", "fs_state", "fs_sum")
    assert tuple(n for n, _ in _CTCBeamStateC._fields_) == STATE_FIELDS          # (the stream state is what it was)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mi355x_asr.h"\nint main(){\n'
           ' printf("%zu", sizeof(mi355x_ctc_beam_fusion));\n'
           + "".join(f' printf(" %zu", offsetof(mi355x_ctc_beam_fusion, {f}));\n' for f in FUSION_FIELDS)
           + ' printf(" %zu", sizeof(mi355x_ctc_beam_fused_state));\n'
           + "".join(f' printf(" %zu", offsetof(mi355x_ctc_beam_fused_state, {f}));\n' for f in ("beams", "fs_state", "fs_sum"))
           + "".join(f' printf(" %zu", offsetof(mi355x_ctc_beam_fused_state, beams.{f}));\n' for f in STATE_FIELDS)
           + " return 0; }\n")
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "t.c"), os.path.join(tmp, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = list(map(int, subprocess.check_output([exe]).decode().split()))
    want = ([ctypes.sizeof(_CTCBeamFusionC)] + [getattr(_CTCBeamFusionC, f).offset for f in FUSION_FIELDS]
            + [ctypes.sizeof(_CTCBeamFusedStateC)] + [getattr(_CTCBeamFusedStateC, f).offset for f in ("beams", "fs_state", "fs_sum")]
            + [_CTCBeamFusedStateC.beams.offset + getattr(_CTCBeamStateC, f).offset for f in STATE_FIELDS])
    assert vals == want


def _keep():
    return [torch.zeros(64, dtype=torch.int64) for _ in range(14)]   # host memory: never dereferenced by a refused call


def _fusion(p, n, **over):
    from nemo_amd.ops import _CTCBeamFusionC
    arr = (_CTCBeamFusionC * max(n, 1))()
    for i in range(max(n, 1)):
        f = dict({k: p(10) for k in FUSION_FIELDS[:6]}, state_final=p(11) if i == n - 1 else None, n_states=2, n_arcs=4, alpha=0.5, ub=1.0)
        if i == over.get("model", 0):
            f.update({k: v for k, v in over.items() if k != "model"})
        arr[i] = _CTCBeamFusionC(**f)
    return arr


def _fused_state(p, base, without=None, second=True):
    from nemo_amd.ops import _CTCBeamFusedStateC, _CTCBeamStateC
    s = _CTCBeamFusedStateC(beams=_CTCBeamStateC(**{f: p(base) for f in STATE_FIELDS if f != without}),
                            fs_state=p(base) if second and without != "fs_state" else None,
                            fs_sum=p(base) if second and without != "fs_sum" else None)
    return s


def _call(stream, n_models=2, fusion=None, **over):
    """a fused entry with plausible non-null arguments (nothing is launched where the arguments are refused) and `over` applied"""
    from nemo_amd import _lib
    keep = _keep()
    p = lambda i: keep[i].data_ptr()
    a = dict(logp=p(0), lens=p(1), ws=p(2), tokens=p(3), tok_frame=p(4), hyp_len=p(5), score=p(6), n_hyp=p(7), B=1, T=2, C=5, blank=4,
             W=4, theta=20.0, beta=0.0, Tcap=8, s_in=_fused_state(p, 8), s_out=_fused_state(p, 9), n=n_models,
             models=_fusion(p, n_models, **(fusion or {})))
    if "s_in_without" in over:
        a["s_in"] = _fused_state(p, 8, over.pop("s_in_without"))
    if "s_out_without" in over:
        a["s_out"] = _fused_state(p, 9, over.pop("s_out_without"))
    a.update(over)
    ref = lambda s: ctypes.byref(s) if s is not None else None
    head = (a["logp"], a["lens"], a["ws"], a["tokens"], a["tok_frame"], a["hyp_len"], a["score"], a["n_hyp"], a["B"], a["T"], a["C"],
            a["blank"], a["W"], a["theta"], a["beta"], ctypes.cast(a["models"], ctypes.c_void_p) if a["models"] is not None else None,
            a["n"])
    if stream:
        return _lib.lib.mi355x_ctc_beam_decode_fused_stream(*head, a["Tcap"], ref(a["s_in"]), ref(a["s_out"]), None)
    return _lib.lib.mi355x_ctc_beam_decode_fused(*head, None)


@pytest.mark.parametrize("stream", [False, True])
def test_bad_arguments_are_refused_before_any_launch(stream):
    bad = [dict(W=65), dict(W=0), dict(C=8193), dict(theta=0.0), dict(theta=float("nan")), dict(beta=float("nan")), dict(logp=None),
           dict(lens=None), dict(ws=None), dict(blank=5), dict(blank=3), dict(T=0), dict(B=0),
           dict(n=0), dict(n=3), dict(n=-1), dict(models=None)]
    if stream:
        bad += [dict(s_out=None), dict(s_out_without="brank"), dict(s_in_without="frames_done"), dict(s_out_without="lm_sum"),
                dict(s_in_without="lm_state"), dict(s_out_without="fs_state"), dict(s_out_without="fs_sum"),
                dict(s_in_without="fs_state"), dict(s_in_without="fs_sum"), dict(Tcap=0), dict(Tcap=0x3fffffff // 4 + 1),
                dict(tokens=None), dict(n_hyp=None, score=None)]
    else:
        bad += [dict(tokens=None), dict(tok_frame=None), dict(hyp_len=None), dict(score=None), dict(n_hyp=None)]
    for over in bad:
        assert _call(stream, **over) == 1, over
    for n_models in (1, 2):
        for model in range(n_models):
            for f in ([dict(alpha=-1.0), dict(alpha=float("nan")), dict(ub=float("nan")), dict(n_states=1), dict(n_arcs=3)]
                      + [{k: None} for k in FUSION_FIELDS[:6]]):
                assert _call(stream, n_models, dict(f, model=model)) == 1, (n_models, model, f)
    if stream:
        keep = _keep()
        same = _fused_state(lambda i: keep[i].data_ptr(), 9)
        assert _call(True, s_in=same, s_out=same) == 1   # in place


# ---------------------------------------------------------------------------------------------- the stream state
def test_stream_state_with_and_without_the_second_model():
    from nemo_amd.modules import CTCBeamStreamState as S
    plain = S.fresh(2, 4, "cpu", lm=True)
    assert plain.fs is None and set(plain.arrays()) == set(STATE_FIELDS) and plain.beams.shape == (10, 2, 4)
    assert plain.next(3).fs is None and S.gather([(plain, 1)]).fs is None
    s = S.fresh(3, 5, "cpu", capacity=16, lm=True, second=True)
    a = s.arrays()
    assert set(a) == set(STATE_FIELDS) | {"fs_state", "fs_sum"} and s.beams.shape == (10, 3, 5)
    assert a["fs_state"].dtype == torch.int32 and a["fs_sum"].dtype == torch.float32 and a["fs_state"].shape == (3, 5)
    assert (a["fs_state"] == 1).all() and (a["fs_sum"] == 0).all()
    n = s.next(7)
    assert n.fs is not None and n.fs is not s.fs and n.fs.shape == s.fs.shape and n.bound == 7
    s.fs[0, 2] = 9
    g = S.gather([(s, 2), (s, 0)])
    assert g.fs.shape == (2, 2, 5) and (g.arrays()["fs_state"][0] == 9).all() and (g.arrays()["fs_state"][1] == 1).all()
    with pytest.raises(ValueError):
        S.gather([(s, 0), (S.fresh(1, 5, "cpu", lm=True), 0)])


def test_state_mismatch_raises_before_any_launch():
    import ctc_beam_lm_oracle as L
    from nemo_amd import ops
    from nemo_amd.modules import CTCBeamStreamState as S, NGramLM
    t = _tree([(0, 1)], 4)
    with tempfile.TemporaryDirectory() as d:
        L.write_arpa(L.make_lm(0, 4, 2), os.path.join(d, "lm.arpa"))
        lm = NGramLM.from_arpa(os.path.join(d, "lm.arpa"), 4)
    logp = torch.zeros(2, 3, 5)
    for state, models in ((S.fresh(2, 4, "cpu", lm=True), [(lm, 0.5), (t, 1.0)]), (S.fresh(2, 4, "cpu", lm=True, second=True), [(t, 1.0)]),
                          (S.fresh(2, 4, "cpu"), [(t, 1.0)]), (S.fresh(3, 4, "cpu", lm=True), [(t, 1.0)])):
        with pytest.raises(ValueError, match="state"):
            ops.ctc_beam_decode_fused_stream(logp, None, 4, 4, 20.0, 0.0, state, models)
