"""No GPU: the oracle of the CTC beam search with n-gram fusion (tests/ctc_beam_lm_oracle.py) against the LM-less oracle and the
exact CTC log-likelihood, `NGramLM` (ARPA reader + back-off automaton) against the oracle's dict recursion, and the plumbing: the
config keys on the three model classes, the refusals that stay, the new ABI symbol and its argument checks."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import ctc_beam_lm_oracle as L
import ctc_beam_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oracle_with_alpha_zero_is_the_lm_less_oracle(dtype):
    for seed, (T, C, W, theta, beta) in enumerate([(20, 5, 4, np.inf, 0.0), (12, 9, 3, 4.0, 0.5), (4, 3, 64, np.inf, 0.25)]):
        lp = O.make_logp(seed, T, C)
        a = O.beam_search(lp, C - 1, W, theta, beta, dtype=dtype)
        b = L.beam_search_lm(lp, C - 1, W, theta, beta, 0.0, L.make_lm(0, C - 1, 3), 3, dtype=dtype)
        assert a["nbest"] == b["nbest"] and a["margin"] == b["margin"] and a["min_candidates"] == b["min_candidates"]
        assert all(type(s) is dtype and x.tobytes() == s.tobytes() for (_, x), (_, s) in zip(a["nbest"], b["nbest"]))


@pytest.mark.parametrize("seed,order,alpha,beta", [(0, 3, 0.5, 0.0), (1, 2, 1.0, 0.5), (2, 1, 0.3, 0.0)])
def test_oracle_is_exact_where_the_beam_holds_every_prefix(seed, order, alpha, beta):
    """T = 4, C = 3, W = 64: all 15 label sequences come out, each scored ctc_loglik + alpha * lm + beta * len"""
    lp = O.make_logp(seed, 4, 3)
    ng = L.make_lm(seed, 2, order)
    r = L.beam_search_lm(lp, 2, 64, np.inf, beta, alpha, ng, order)
    feasible = [p for U in range(5) for p in itertools.product((0, 1), repeat=U) if np.isfinite(O.ctc_loglik(lp, list(p), 2))]
    assert len(feasible) == 15 and sorted(p for p, _ in r["nbest"]) == sorted(feasible) and r["margin"] == np.inf
    scores = [s for _, s in r["nbest"]]
    assert scores == sorted(scores, reverse=True)
    for p, s in r["nbest"]:
        assert abs(float(s) - (O.ctc_loglik(lp, list(p), 2) + alpha * L.lm_score(ng, order, p) + beta * len(p))) <= 1e-12, p
    assert L.lm_score(ng, order, ()) == 0.0


def test_oracle_rows_are_the_textbook_recursion():
    """the vectorised conditional rows the search uses against the one-value recursion, float64 exactly the same sums up to their
    association, float32 within rounding"""
    ng = L.make_lm(0, 28, 3)
    r64, r32 = L._Rows(ng, 3, 28, np.float64), L._Rows(ng, 3, 28, np.float32)
    ctxs = [(), (L.BOS,), (3,), (L.BOS, 5)] + [g for g in ng if len(g) == 2][:40] + [(1, 2), (27, 27)]
    for ctx in ctxs:
        ctx = ctx[-2:]
        want = np.array([L.cond_logp(ng, ctx, c) for c in range(28)])
        assert np.abs(r64.cond_row(ctx) - want).max() <= 1e-12
        assert r32.cond_row(ctx).dtype == np.float32 and np.abs(r32.cond_row(ctx) - want).max() <= 2e-6


# ---------------------------------------------------------------------------------------------- NGramLM against the dict recursion
def _words(V):
    return [f"w{i}" for i in range(V)]


def _load(ng, V, tmp_path, by_vocabulary):
    from nemo_amd.modules import NGramLM
    path = tmp_path / f"lm_{V}_{int(by_vocabulary)}.arpa"
    if by_vocabulary:
        L.write_arpa(ng, path, token_offset=None, vocabulary=_words(V))
        return NGramLM.from_arpa(path, V, token_offset=None, vocabulary=_words(V))
    L.write_arpa(ng, path, token_offset=100)
    return NGramLM.from_arpa(path, V)


def _hit_order(ng, order, ids, k):
    """the order of the n-gram that scores ids[k]: order = found without backing off, 1 = backed off through every level"""
    g = L.context_of(ids[:k], order) + (ids[k],)
    while g not in ng:
        g = g[1:]
    return len(g)


@pytest.mark.parametrize("by_vocabulary", [False, True])
@pytest.mark.parametrize("V,order", [(4, 3), (28, 3), (128, 4), (1024, 3)])
def test_flattened_tables_score_like_the_dict(V, order, by_vocabulary, tmp_path):
    ng = L.make_lm(0, V, order)
    lm = _load(ng, V, tmp_path, by_vocabulary)
    n_states = 2 + sum(1 for g in ng if len(g) < order and g != (L.BOS,))
    assert (lm.order, lm.vocab_size, lm.num_states, lm.num_arcs) == (order, V, n_states, len(ng) - 1)
    # state 0: V arcs, arc c = label c, the unigram values
    assert lm.state_arc_begin[0] == 0 and lm.state_arc_begin[1] == V and lm.arc_tok[:V].tolist() == list(range(V))
    assert np.array_equal(lm.arc_logp[:V], np.array([np.float32(ng[(c,)][0] * L.LN10) for c in range(V)], dtype=np.float32))
    assert lm.state_bo_next[1] == 0 and lm.state_bo[1] == np.float32(ng[(L.BOS,)][1] * L.LN10)
    for a in (lm.state_arc_begin, lm.arc_tok, lm.arc_next, lm.state_bo_next):
        assert a.dtype == np.int32 and a.flags.c_contiguous
    assert lm.arc_logp.dtype == lm.state_bo.dtype == np.float32
    # 200 sequences: random ones, and n-grams of the file behind a random token (found at every order without backing off)
    rng = np.random.default_rng(V + order)
    top = [g for g in ng if len(g) == order and g[0] != L.BOS]
    seqs = [tuple(int(x) for x in rng.integers(V, size=int(rng.integers(1, 13)))) for _ in range(150)]
    seqs += [(int(rng.integers(V)),) + top[int(rng.integers(len(top)))] + (int(rng.integers(V)),) for _ in range(50)]
    hit = set()
    for ids in seqs:
        want = L.lm_score(ng, order, ids)
        assert abs(lm.score(ids) - want) <= 1e-5 * abs(want), ids
        hit |= {_hit_order(ng, order, ids, k) for k in range(len(ids))}
    assert hit == set(range(1, order + 1)), hit   # every level of the back-off chain was walked
    assert lm.score(()) == 0.0


@pytest.mark.parametrize("V", [4, 28])
def test_lm_ub_bounds_every_conditional(V, tmp_path):
    """a full sweep: every label behind every history of up to 3 tokens (from <s>, which reaches every context of a trigram model),
    the table walk against the dict recursion, and lm_ub above all of them; the generator has positive back-off weights"""
    ng = L.make_lm(0, V, 3)
    assert any(bo > 0 for _, bo in ng.values())
    lm = _load(ng, V, tmp_path, False)
    largest, n = -np.inf, 0
    for h in itertools.chain.from_iterable(itertools.product(range(V), repeat=k) for k in range(3)):
        s = 1
        for c in h:
            _, s = lm.lookup(s, c)
        for c in range(V):
            v, _ = lm.lookup(s, c)
            want = L.cond_logp(ng, L.context_of(h, 3), c)
            assert abs(v - want) <= 1e-5 * max(1.0, abs(want)), (h, c)
            largest, n = max(largest, v), n + 1
    assert n == (1 + V + V * V) * V and lm.lm_ub >= largest + 5e-4   # (the bound carries a slack of 1e-3 for float32 sums)


# ---------------------------------------------------------------------------------------------- what the reader refuses
GOOD = ["\\data\\", "ngram 1=4", "ngram 2=2", "", "\\1-grams:", "-1.0\t<s>\t-0.5", "-0.5\td\t-0.25", "-0.7\te\t-0.1", "-2.0\t<unk>", "",
        "\\2-grams:", "-0.3\t<s> d", "-0.4\td e", "", "\\end\\"]


def _write(tmp_path, lines, name="m.arpa"):
    p = tmp_path / name
    p.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return p


def test_reader_accepts_a_small_file_and_fills_labels_from_unk(tmp_path):
    from nemo_amd.modules import NGramLM
    lm = NGramLM.from_arpa(_write(tmp_path, GOOD), 3)   # labels d, e, f = chr(100 ..): f has no unigram and gets <unk>'s
    ln10 = L.LN10
    assert lm.order == 2 and lm.num_states == 5 and lm.num_arcs == 5
    assert abs(lm.score([0]) - (-0.3 * ln10)) < 1e-6 and abs(lm.score([0, 1]) - (-0.7 * ln10)) < 1e-6
    assert abs(lm.score([2]) - ((-0.5 - 2.0) * ln10)) < 1e-6          # backoff(<s>) + <unk>
    assert abs(lm.score([1, 0]) - ((-0.5 - 0.7 - 0.1 - 0.5) * ln10)) < 1e-6   # e: bo(<s>) + p(e); then d: bo(e) + p(d)
    # space-separated fields are read as well; n-grams with </s> are dropped
    spaced = [l.replace("\t", " ") for l in GOOD]
    spaced[1], spaced[2] = "ngram 1=5", "ngram 2=3"
    spaced.insert(9, "-1.5 </s>")
    spaced.insert(14, "-0.2 e </s>")
    lm2 = NGramLM.from_arpa(_write(tmp_path, spaced, "s.arpa"), 3)
    assert lm2.num_arcs == 5 and all(np.array_equal(getattr(lm, a), getattr(lm2, a)) for a in ("arc_tok", "arc_logp", "arc_next", "state_bo"))


@pytest.mark.parametrize("edit,what", [
    (lambda g: g.__setitem__(1, "ngram 1=5"), "announces 5 1-grams"),           # count mismatch with \data\
    (lambda g: g.__setitem__(12, "-0.4\td z"), r":13: unknown word 'z'"),       # a word that is no label
    (lambda g: g.__setitem__(6, "nan\td\t-0.25"), r":7: non-finite"),
    (lambda g: g.__setitem__(6, "-0.5\td\tinf"), r":7: non-finite"),
    (lambda g: g.__setitem__(6, "-0.5x\td"), r":7: .*not a number"),
    (lambda g: g.__setitem__(12, "-0.4\td <s>"), r":13: <s> behind the first word"),
    (lambda g: g.__setitem__(12, "-0.4\td"), r":13: 1 words in the 2-grams"),
    (lambda g: g.__setitem__(12, "-0.3\t<s> d"), r":13: .*twice"),
    (lambda g: g.pop(), "not an ARPA file"),
    (lambda g: g.__setitem__(10, "\\3-grams:"), r":11: unexpected section"),
])
def test_malformed_files_raise_naming_the_line(edit, what, tmp_path):
    from nemo_amd.modules import NGramLM
    lines = list(GOOD)
    edit(lines)
    with pytest.raises(ValueError, match=what):
        NGramLM.from_arpa(_write(tmp_path, lines), 3)


def test_a_missing_unigram_without_unk_raises(tmp_path):
    from nemo_amd.modules import NGramLM
    lines = [l for l in GOOD if "<unk>" not in l]
    lines[1] = "ngram 1=3"
    with pytest.raises(ValueError, match="label 2 has no unigram.*<unk>"):
        NGramLM.from_arpa(_write(tmp_path, lines), 3)
    assert NGramLM.from_arpa(_write(tmp_path, lines), 2).num_arcs == 4   # (with two labels nothing is missing)
    with pytest.raises(ValueError, match="vocabulary"):
        NGramLM.from_arpa(_write(tmp_path, lines), 2, token_offset=None)
    with pytest.raises(ValueError, match="cannot be words"):
        NGramLM.from_arpa(_write(tmp_path, lines), 2, token_offset=None, vocabulary=["d", " "])


def test_tables_that_break_the_rules_are_refused():
    from nemo_amd.modules import NGramLM
    lm = NGramLM._from_ngrams({g: tuple(v) for g, v in L.make_lm(0, 4, 3).items()}, 3, 4, None)
    tables = dict(state_arc_begin=lm.state_arc_begin, arc_tok=lm.arc_tok, arc_logp=lm.arc_logp, arc_next=lm.arc_next,
                  state_bo=lm.state_bo, state_bo_next=lm.state_bo_next, state_len=lm.state_len)
    assert NGramLM(4, 3, **tables).lm_ub == lm.lm_ub

    def broken(name, idx, value):
        t = {k: v.copy() for k, v in tables.items()}
        t[name][idx] = value
        return t
    S, A = lm.num_states, lm.num_arcs
    for name, idx, value in (("arc_next", 5, S), ("arc_next", 5, -1), ("state_bo_next", 3, S), ("state_bo_next", 2, 2),
                             ("arc_tok", 2, 3), ("arc_tok", A - 1, 4), ("state_arc_begin", 1, 3), ("state_arc_begin", S, A + 1),
                             ("arc_logp", 0, np.nan), ("state_bo", 1, np.inf)):
        with pytest.raises(ValueError, match="n-gram LM"):
            NGramLM(4, 3, **broken(name, idx, value))
    begin = lm.state_arc_begin
    s = next(k for k in range(1, S) if begin[k + 1] - begin[k] >= 2)   # a state with two arcs: swap them
    t = {k: v.copy() for k, v in tables.items()}
    t["arc_tok"][[begin[s], begin[s] + 1]] = t["arc_tok"][[begin[s] + 1, begin[s]]]
    with pytest.raises(ValueError, match="not sorted"):
        NGramLM(4, 3, **t)


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


def _arpa(tmp_path, V, order=3, name="lm.arpa"):
    ng = L.make_lm(0, V, order)
    L.write_arpa(ng, tmp_path / name)
    return str(tmp_path / name), ng


def _beam(path, **kw):
    return dict(strategy="beam_batch", beam=dict(beam_size=4, ngram_lm_arpa=path, ngram_lm_alpha=0.4, **kw))


def test_ngram_lm_arpa_is_accepted_by_the_ctc_model(tmp_path):
    from nemo_amd.models import EncDecCTCModel
    from nemo_amd.modules import BeamBatchedCTCDecoder, NGramLM, ctc_decoder_from_config
    path, ng = _arpa(tmp_path, len(VOCAB))
    dec = EncDecCTCModel(_ctc_cfg(**_beam(path))).wer.decoding
    assert isinstance(dec, BeamBatchedCTCDecoder) and isinstance(dec.ngram_lm, NGramLM) and dec.ngram_lm_alpha == 0.4
    assert dec.ngram_lm.vocab_size == len(VOCAB) == dec.blank_id and dec.ngram_lm.order == 3
    assert abs(dec.ngram_lm.score([7, 4, 11]) - L.lm_score(ng, 3, (7, 4, 11))) < 1e-5
    # an NGramLM in the place of the path; alpha defaults to 0; without the key there is no LM
    same = ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(ngram_lm_arpa=dec.ngram_lm)), VOCAB)
    assert same.ngram_lm is dec.ngram_lm and same.ngram_lm_alpha == 0.0
    assert ctc_decoder_from_config(dict(strategy="beam_batch"), VOCAB).ngram_lm is None
    # words = the vocabulary's strings: refused for this vocabulary (it has a blank as a label), accepted for one without
    with pytest.raises(ValueError, match="cannot be words"):
        ctc_decoder_from_config(_beam(path, ngram_lm_token_offset=None), VOCAB)
    L.write_arpa(L.make_lm(0, 26, 2), tmp_path / "w.arpa", token_offset=None, vocabulary=VOCAB[:26])
    byw = ctc_decoder_from_config(_beam(str(tmp_path / "w.arpa"), ngram_lm_token_offset=None), VOCAB[:26])
    assert byw.ngram_lm.order == 2 and byw.ngram_lm.vocab_size == 26
    with pytest.raises(ValueError, match="labels"):   # an LM over another label set
        ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(ngram_lm_arpa=byw.ngram_lm)), VOCAB)
    with pytest.raises(FileNotFoundError, match="ngram_lm_arpa"):
        EncDecCTCModel(_ctc_cfg(**_beam(str(tmp_path / "absent.arpa")))).wer
    with pytest.raises(NotImplementedError, match="timestamps"):
        EncDecCTCModel(_ctc_cfg(**_beam(path))).transcribe([np.zeros(1600, dtype=np.float32)], timestamps=True)
    with pytest.raises(NotImplementedError, match="confidence_cfg"):
        EncDecCTCModel(_ctc_cfg(confidence_cfg=dict(preserve_token_confidence=True), **_beam(path))).wer


def test_ngram_lm_arpa_is_accepted_by_the_bpe_model(tmp_path):
    from nemo_amd.models import EncDecCTCModelBPE
    from nemo_amd.modules import BeamBatchedCTCDecoder
    from test_abi_and_host import _train_spm
    words = ["hello", "world", "speech", "model", "conformer", "audio", "signal", "frame", "token", "layer", "attention", "gradient"]
    path, _ = _arpa(tmp_path, 64, order=2)
    cfg = _ctc_cfg(**_beam(path))
    cfg["decoder"].update(vocabulary=None, num_classes=-1)
    cfg.pop("labels")
    cfg["tokenizer"] = dict(dir=_train_spm(tmp_path, "tok64", 64, words), type="bpe")
    dec = EncDecCTCModelBPE(cfg).wer.decoding
    assert isinstance(dec, BeamBatchedCTCDecoder) and dec.blank_id == 64 and dec.ngram_lm.vocab_size == 64 and dec.ngram_lm_alpha == 0.4


def test_ngram_lm_arpa_is_accepted_by_the_hybrid_model(tmp_path):
    from nemo_amd.models import EncDecHybridRNNTCTCModel
    from nemo_amd.modules import BeamBatchedCTCDecoder, GreedyCTCDecoder
    path, _ = _arpa(tmp_path, len(VOCAB))
    m = EncDecHybridRNNTCTCModel(_hybrid_cfg(**_beam(path)))
    assert isinstance(m.ctc_decoding, BeamBatchedCTCDecoder) and m.ctc_decoding.ngram_lm.order == 3 and m.ctc_decoding.ngram_lm_alpha == 0.4
    m = EncDecHybridRNNTCTCModel(_hybrid_cfg())
    with pytest.raises(FileNotFoundError, match="ngram_lm_arpa"):   # refused before anything is replaced
        m.change_decoding_strategy(_beam(str(tmp_path / "absent.arpa")), decoder_type="ctc")
    assert isinstance(m.ctc_decoding, GreedyCTCDecoder) and m.cur_decoder == "rnnt"
    m.change_decoding_strategy(_beam(path), decoder_type="ctc")
    assert m.cur_decoder == "ctc" and m.ctc_decoding.ngram_lm is not None and m.ctc_decoding.ngram_lm.vocab_size == len(VOCAB)


@pytest.mark.parametrize("beam,name", [(dict(ngram_lm_model="lm.arpa"), "ngram_lm_model"), (dict(kenlm_path="lm.bin"), "kenlm_path"),
                                       (dict(ngram_lm_alpha=0.3), "ngram_lm_alpha")])
def test_the_three_refusals_stay(beam, name, tmp_path):
    from nemo_amd.models import EncDecCTCModel, EncDecHybridRNNTCTCModel
    from nemo_amd.modules import ctc_decoder_from_config
    with pytest.raises(NotImplementedError, match=name):
        EncDecCTCModel(_ctc_cfg(strategy="beam_batch", beam=beam)).wer
    with pytest.raises(NotImplementedError, match=name):
        EncDecHybridRNNTCTCModel(_hybrid_cfg(strategy="beam_batch", beam=beam))
    if name != "ngram_lm_alpha":   # also beside a readable ARPA file; and the message points to the key that is read
        path, _ = _arpa(tmp_path, len(VOCAB))
        with pytest.raises(NotImplementedError, match=f"{name}.*ngram_lm_arpa"):
            ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(beam, ngram_lm_arpa=path)), VOCAB)


def test_negative_alpha_raises(tmp_path):
    from nemo_amd.modules import BeamBatchedCTCDecoder, NGramLM, ctc_decoder_from_config
    path, _ = _arpa(tmp_path, len(VOCAB))
    lm = NGramLM.from_arpa(path, len(VOCAB))
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="ngram_lm_alpha"):
            BeamBatchedCTCDecoder(VOCAB, ngram_lm=lm, ngram_lm_alpha=bad)
    with pytest.raises(ValueError, match="ngram_lm_alpha"):
        ctc_decoder_from_config(dict(strategy="beam_batch", beam=dict(ngram_lm_arpa=path, ngram_lm_alpha=-1.0)), VOCAB)
    with pytest.raises(TypeError, match="NGramLM"):
        BeamBatchedCTCDecoder(VOCAB, ngram_lm=path)
    with pytest.raises(ValueError, match="labels"):
        BeamBatchedCTCDecoder(VOCAB[:5], ngram_lm=lm)


# ---------------------------------------------------------------------------------------------- the ABI
def test_lm_symbol_is_exported_declared_and_checks_its_arguments():
    from nemo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi355x_asr.h")).read()
    declared = set(re.findall(r"\b(mi355x_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = "mi355x_ctc_beam_decode_lm"
    assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert len(_lib.SIGNATURES[name]) == 26 and len(_lib.SIGNATURES["mi355x_ctc_beam_decode"]) == 16   # the old entry keeps its signature
    assert _lib.SIGNATURES[name][:15] == _lib.SIGNATURES["mi355x_ctc_beam_decode"][:15]
    # argument checks return MI_ERR_ARG (1) before anything is launched: the pointers are never followed
    p = 4096   # non-null, 8-byte aligned
    ok = dict(logp=p, lens=p, ws=p, tokens=p, tok_frame=p, hyp_len=p, score=p, n_hyp=p, B=2, T=8, C=5, blank=4, beam=4, thr=20.0, beta=0.0,
              begin=p, arc_tok=p, arc_logp=p, arc_next=p, bo=p, bo_next=p, S=2, A=4, alpha=0.5, ub=0.0)
    order = list(ok)

    def rc(**kw):
        a = dict(ok, **kw)
        return _lib.lib.mi355x_ctc_beam_decode_lm(*(a[k] for k in order), None)
    for ptr in ("logp", "lens", "ws", "tokens", "tok_frame", "hyp_len", "score", "n_hyp", "begin", "arc_tok", "arc_logp", "arc_next", "bo",
                "bo_next"):
        assert rc(**{ptr: None}) == 1, ptr
    for bad in (dict(S=1), dict(S=0), dict(S=-3), dict(A=3), dict(A=-1), dict(blank=3), dict(blank=0), dict(alpha=-0.5),
                dict(alpha=float("nan")), dict(alpha=-float("inf")), dict(ub=float("nan")),
                # what the LM-less entry refuses is refused here as well
                dict(beam=0), dict(beam=65), dict(blank=-1), dict(blank=5), dict(thr=0.0), dict(thr=float("nan")), dict(B=0), dict(T=0),
                dict(C=0), dict(C=8193, blank=8192, A=8192), dict(ws=p + 4), dict(beta=float("nan"))):
        assert rc(**bad) == 1, bad
