"""-m gpu: `mi355x_ctc_beam_decode` against the float64 oracle of the search (tests/ctc_beam_oracle.py), and `strategy: beam_batch`
through the decoding object, the CTC model and the hybrid model's CTC head.

Parity rule.  float32 sums cannot reproduce a float64 selection through a near-tie, so a (shape, seed) case is compared only if the
oracle's cut margin -- min over the frames of rank[W-1] - rank[W] -- is >= 1e-3 (a condition on the input, not a measurement of the
device; the float32 restatement of the oracle differs from float64 by <= 7e-5 on every shape here).  Seeds 0..23 are taken per
shape and at least 5 must pass the rule, else the test FAILS.  Kept with the generator of the oracle module: 23, 18, 18, 24, 19, 15,
14 seeds for the first seven shapes, 8 at (12, 1025, 64, 6) and 6 at (24, 70, 64, inf).

In a kept case: the device's set of hypotheses equals the oracle's, n_hyp and hyp_len are equal, device scores are non-increasing,
each score is within max(8 * e32, 16 ulp of the score) of float64 where e32 is the float32 restatement's own largest error on that
case (reference against reference, never the device), every tok_frame is strictly increasing along its hypothesis and lies in
[0, len), and the -1 / -inf padding is exact."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
MARGIN = 1e-3
VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]

# (T, C, W, threshold, beta); blank = C - 1
SHAPES = [
    (37, 5, 4, INF, 0.0),       # C < 64
    (70, 29, 8, INF, 0.0),      # crossing 64 frames
    (200, 33, 3, INF, 0.0),     # W not a power of two, long chase
    (130, 129, 1, INF, 0.0),    # W = 1
    (24, 129, 16, 8.0, 0.0),    # C in three groups of 64, finite threshold
    (24, 129, 16, 8.0, 0.5),    # the same with beta != 0
    (66, 129, 8, 8.0, 0.5),     # beta with a longer walk
    # full wave, BPE width.  T = 12, shortened from 16: at T = 16 only seeds 18 and 23 of 0..23 have a cut margin >= 1e-3, at
    # T = 12 eight do (1, 8, 10, 12, 15, 18, 22, 23); every frame still has > 700 candidates for the 64 places
    (12, 1025, 64, 6.0, 0.0),
    (24, 70, 64, INF, 0.0),     # full wave, no pruning (6 seeds kept at the T the shape was given with)
]


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


@functools.lru_cache(maxsize=None)
def _reference(seed, T, C, W, theta, beta):
    """(logp, float64 result, float32 result or None) of one utterance; the float32 run only where the case is kept"""
    lp = O.make_logp(seed, T, C)
    r64 = O.beam_search(lp, C - 1, W, theta, beta)
    r32 = O.beam_search(lp, C - 1, W, theta, beta, dtype=np.float32) if r64["margin"] >= MARGIN else None
    return lp, r64, r32


def _e32(r64, r32):
    d64 = dict(r64["nbest"])
    common = [abs(float(s) - float(d64[p])) for p, s in r32["nbest"] if p in d64]
    return max(common) if common else 0.0


def _decode(logp, lens, W, theta, beta):
    from nemo_amd import ops
    out = ops.ctc_beam_decode(torch.from_numpy(np.ascontiguousarray(logp)).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev),
                              logp.shape[2] - 1, W, theta, beta)
    torch.cuda.synchronize()
    tokens, tok_frame, hyp_len, score, n_hyp = (t.cpu().numpy() for t in out)
    assert tokens.dtype == tok_frame.dtype == hyp_len.dtype == n_hyp.dtype == np.int32 and score.dtype == np.float32
    assert tokens.shape == tok_frame.shape == (logp.shape[0], W, logp.shape[1]) and score.shape == hyp_len.shape == (logp.shape[0], W)
    return tokens, tok_frame, hyp_len, score, n_hyp


def _check_row(tag, T, W, tokens, tok_frame, hyp_len, score, n_hyp, expect, e32):
    """one utterance of the device's output against `expect` = {token tuple: float64 score}; -> its largest score error and bound"""
    n = int(n_hyp)
    assert n == len(expect), (tag, n, len(expect))
    got = [tuple(tokens[k, : hyp_len[k]].tolist()) for k in range(n)]
    assert len(set(got)) == n and set(got) == set(expect), (tag, set(got) ^ set(expect))
    assert all(score[k] >= score[k + 1] for k in range(n - 1)), (tag, score[:n])
    worst, bound = 0.0, 0.0
    for k, p in enumerate(got):
        assert hyp_len[k] == len(p)
        err, tol = abs(float(score[k]) - float(expect[p])), max(8 * e32, 16 * _ulp(expect[p]))
        if err / tol >= worst / max(bound, 1e-300) or bound == 0.0:
            worst, bound = err, tol
        assert err <= tol, (tag, p, float(score[k]), float(expect[p]), err, tol)
        fr = tok_frame[k, : len(p)]
        assert (np.diff(fr) > 0).all() and (len(p) == 0 or (fr[0] >= 0 and fr[-1] < T)), (tag, p, fr)
        assert (tokens[k, len(p):] == -1).all() and (tok_frame[k, len(p):] == -1).all(), (tag, k)
    assert (tokens[n:] == -1).all() and (tok_frame[n:] == -1).all() and (hyp_len[n:] == 0).all() and np.isneginf(score[n:]).all(), tag
    return worst, bound


@pytest.mark.parametrize("T,C,W,theta,beta", SHAPES)
def test_beam_search_matches_the_oracle(T, C, W, theta, beta):
    kept = [s for s in range(24) if _reference(s, T, C, W, theta, beta)[2] is not None]
    print(f"CTC_BEAM kept T={T} C={C} W={W} theta={theta} beta={beta}: {len(kept)} of 24 seeds {kept}")
    assert len(kept) >= 5, kept
    refs = [_reference(s, T, C, W, theta, beta) for s in kept]
    if W == 64:   # the full wave has something to cut in every frame
        assert all(r64["min_candidates"] > W for _, r64, _ in refs), [r64["min_candidates"] for _, r64, _ in refs]
    logp = np.stack([lp for lp, _, _ in refs])
    out = _decode(logp, [T] * len(kept), W, theta, beta)
    worst = (0.0, 0.0)
    for b, (seed, (_, r64, r32)) in enumerate(zip(kept, refs)):
        e32 = _e32(r64, r32)
        w = _check_row((T, C, W, theta, beta, seed), T, W, *(o[b] for o in out), dict(r64["nbest"]), e32)
        if w[0] / max(w[1], 1e-300) >= worst[0] / max(worst[1], 1e-300):
            worst = w
    print(f"CTC_BEAM err T={T} C={C} W={W} theta={theta} beta={beta}: largest score error {worst[0]:.3e} against its bound {worst[1]:.3e}")


def _first_kept(T, C, W, start=0):
    """the first seed from `start` whose utterance of T frames has a cut margin >= 1e-3 (or is never cut)"""
    for s in range(start, start + 64):
        if _reference(s, T, C, W, INF, 0.0)[2] is not None:
            return s
    raise AssertionError("no seed passes the cut-margin rule")


def test_ragged_batch_junk_beyond_the_lengths_and_the_exhaustive_case():
    """one batch, C = 3, W = 64: lengths {T, T-1, 1, 0} with NaN beyond each length, and the exhaustive case T = 4 (all 15 prefixes,
    every score the exact float64 CTC log-likelihood of its tokens: no margin needed).  Rows of one batch that come out like their
    own single-utterance oracle are independent of each other."""
    T, C, W = 11, 3, 64
    lens = [T, T - 1, 1, 0, 4]
    seeds = [_first_kept(T, C, W), _first_kept(T - 1, C, W, 100), 7, 0, 3]
    logp = np.full((len(lens), T, C), np.nan, dtype=np.float32)
    refs = []
    for b, (n, s) in enumerate(zip(lens, seeds)):
        if n:
            lp, r64, r32 = _reference(s, n, C, W, INF, 0.0)
            logp[b, :n] = lp
        else:
            r64 = r32 = dict(nbest=[((), 0.0)], margin=np.inf, min_candidates=0)
        assert r32 is not None
        refs.append((r64, r32))
    assert len(refs[0][0]["nbest"]) == W and len(refs[1][0]["nbest"]) == W   # the long rows fill the wave: they were cut
    out = _decode(logp, lens, W, INF, 0.0)
    for b, (r64, r32) in enumerate(refs):
        err, tol = _check_row(("ragged", b), lens[b], W, *(o[b] for o in out), dict(r64["nbest"]), _e32(r64, r32))
        print(f"CTC_BEAM ragged row {b} len={lens[b]}: n_hyp={out[4][b]} err={err:.3e} tol={tol:.3e}")
    assert out[4].tolist()[2:] == [2 + 1, 1, 15]   # one frame: the empty prefix and the two labels; no frame: the empty prefix, score 0
    assert out[3][3, 0] == 0.0 and out[2][3, 0] == 0
    # the exhaustive row against the exact likelihood
    lp4, r64, r32 = _reference(3, 4, C, W, INF, 0.0)
    exact = {p: O.ctc_loglik(lp4, list(p), C - 1) for p, _ in r64["nbest"]}
    assert len(exact) == 15
    _check_row("exhaustive", 4, W, *(o[4] for o in out), exact, _e32(r64, r32))
    assert abs(np.exp(out[3][4, :15].astype(np.float64)).sum() - 1.0) < 1e-5


def test_bad_arguments_raise():
    from nemo_amd import ops
    lp = torch.zeros(1, 4, 5, device=dev)
    lens = torch.tensor([4], device=dev)
    for kw in (dict(beam_size=0), dict(beam_size=65), dict(beam_size=4, beam_threshold=0.0), dict(beam_size=4, blank=5)):
        args = dict(blank=4, beam_size=4, beam_threshold=20.0, beam_beta=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.ctc_beam_decode(lp, lens, **args)


# ---------------------------------------------------------------------------------------------- decoding object and models
def test_decoder_texts_and_wer():
    from nemo_amd.modules import WER, BeamBatchedCTCDecoder
    T, C, W = 24, len(VOCAB) + 1, 4
    seeds = [s for s in range(24) if _reference(s, T, C, W, 8.0, 0.0)[2] is not None][:3]
    refs = [_reference(s, T, C, W, 8.0, 0.0) for s in seeds]
    logp = torch.from_numpy(np.stack([r[0] for r in refs])).to(dev)
    lens = torch.full((len(seeds),), T, dtype=torch.int64, device=dev)
    text = lambda p: "".join(VOCAB[i] for i in p)   # noqa: E731
    best = [text(r[1]["nbest"][0][0]) for r in refs]
    dec = BeamBatchedCTCDecoder(VOCAB, beam_size=W, beam_threshold=8.0)
    assert dec(logp, lens) == best and dec.best_texts(logp, lens) == best
    nb = BeamBatchedCTCDecoder(VOCAB, beam_size=W, beam_threshold=8.0, return_best_hypothesis=False)
    lists = nb(logp, lens)
    assert [l[0] for l in lists] == best and all(1 <= len(l) <= W for l in lists)
    assert [set(l) for l in lists] == [set(text(p) for p, _ in r[1]["nbest"]) for r in refs]
    wer = WER(nb)   # scores the best hypothesis, whatever the object returns when called
    tg = torch.zeros(len(seeds), 8, dtype=torch.int64)
    tl = torch.zeros(len(seeds), dtype=torch.int64)
    for b, r in enumerate(refs):
        ids = list(r[1]["nbest"][0][0])[:8]
        tg[b, : len(ids)] = torch.tensor(ids, dtype=torch.int64)
        tl[b] = len(ids)
    wer.update(logp, lens, tg.to(dev), tl.to(dev))
    refs_txt = [text(tg[b, : int(tl[b])].tolist()) for b in range(len(seeds))]
    from oracle import decode_ref as D
    assert abs(wer.compute()[0] - D.word_error_rate(best, refs_txt)) < 1e-12


def _waves():
    g = torch.Generator().manual_seed(7)
    return [0.1 * torch.randn(16000, generator=g), 0.1 * torch.randn(9600, generator=g)]


def _ctc_model(decoding):
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    torch.manual_seed(3)
    cfg = conformer_ctc_config("small", vocab_size=len(VOCAB), d_model=64, n_heads=4, n_layers=2, dropout=0.0,
                               dropout_pre_encoder=0.0, dropout_att=0.0)
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["vocabulary"] = VOCAB
    cfg["labels"] = VOCAB
    cfg["decoding"] = decoding
    m = EncDecCTCModel(cfg)
    with torch.no_grad():
        m.decoder.decoder_layers[0].bias[-1] -= 3.0   # random weights with fewer blanks: the hypotheses are not empty
    return m.to(dev).eval()


def _hybrid_model():
    from nemo_amd.models import EncDecHybridRNNTCTCModel, fastconformer_hybrid_config
    torch.manual_seed(4)
    cfg = fastconformer_hybrid_config("small", vocab_size=len(VOCAB), ctc_loss_weight=0.3, d_model=64, n_heads=4, n_layers=2,
                                      subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0,
                                      compute_dtype=torch.float32)
    cfg["labels"] = VOCAB
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    m = EncDecHybridRNNTCTCModel(cfg)
    with torch.no_grad():
        m.ctc_decoder.decoder_layers[0].bias[-1] -= 3.0
    return m.to(dev).eval()


def _check_model(model, waves):
    """transcribe under beam_batch = the decoding object on the model's own log-probabilities"""
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    dec = model._ctc_decoding()
    assert type(dec).__name__ == "BeamBatchedCTCDecoder" and dec.beam_size == 4 and not dec.return_best_hypothesis
    with torch.no_grad(), _inference_setup(model):
        lp, n = model._ctc_log_probs(*_audio_batch(model, waves))
    want = dec.nbest(lp, n)
    lists = model.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert len(lists) == len(waves) and any(ids for l in lists for _, ids, _ in l)
    for l, w in zip(lists, want):
        assert 1 <= len(l) <= 4 and [(ids, s) for _, ids, s in l] == w
        assert [t for t, _, _ in l] == [dec.ids_to_text(ids) for ids, _ in w]
        assert all(a[2] >= b[2] for a, b in zip(l, l[1:]))   # best first
    assert model.transcribe(waves, batch_size=2) == [[t for t, _, _ in l] for l in lists]
    dec.return_best_hypothesis = True
    try:
        assert model.transcribe(waves, batch_size=2) == [l[0][0] for l in lists]
        assert model.transcribe(waves, batch_size=2, return_hypotheses=True) == [l[0] for l in lists]
    finally:
        dec.return_best_hypothesis = False
    with pytest.raises(NotImplementedError, match="timestamps"):
        model.transcribe(waves, timestamps=True)
    assert all(a["feasible"] for a in model.align(waves, ["abc", "de"]))   # forced alignment is unaffected
    return lists


BEAM4 = dict(strategy="beam_batch", beam=dict(beam_size=4, return_best_hypothesis=False))


def test_ctc_model_transcribes_with_the_beam_search():
    model = _ctc_model(BEAM4)
    lists = _check_model(model, _waves())
    # predict_step scores the best hypothesis
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    with torch.no_grad(), _inference_setup(model):
        sig, lens = _audio_batch(model, _waves())
        pred = model.predict_step((sig, lens, None, None, [0, 1]))
    assert [t for _, t in pred] == [l[0][0] for l in lists]


def test_hybrid_ctc_head_transcribes_with_the_beam_search():
    model = _hybrid_model()
    model.change_decoding_strategy(BEAM4, decoder_type="ctc")
    lists = _check_model(model, _waves())
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    with torch.no_grad(), _inference_setup(model):
        sig, lens = _audio_batch(model, _waves())
        pred = model.predict_step((sig, lens, None, None, [0, 1]))
    assert [t for _, t in pred] == [l[0][0] for l in lists]
    model.change_decoding_strategy(dict(strategy="greedy"), decoder_type="ctc")
    assert all(isinstance(t, str) for t in model.transcribe(_waves(), batch_size=2))


def test_greedy_path_is_what_it_was():
    """the greedy decoding object behind the shared factory: tokens and lengths equal the restated reference loop, and the bits of
    all three outputs equal the kernel entry called directly"""
    from nemo_amd import ops
    from nemo_amd.modules import GreedyCTCDecoder, ctc_decoder_from_config
    from oracle import decode_ref as D
    g = torch.Generator().manual_seed(41)
    B, T, V = 5, 301, 28
    x = torch.randn(B, T, V + 1, generator=g)
    x[:, :, V] += 1.5
    x[1, 40:90] = x[1, 40:41]
    logp = torch.log_softmax(x, -1)
    lens = torch.tensor([T, 250, 301, 0, 17])
    ref = D.greedy_decode(logp, lens, blank=V)
    dec = ctc_decoder_from_config(dict(strategy="greedy_batch"), VOCAB)
    assert type(dec) is GreedyCTCDecoder
    tok, olen, score = dec.decode_ids(logp.to(dev), lens.to(dev))
    raw = ops.ctc_greedy_decode(logp.to(dev), lens.to(dev), V)
    torch.cuda.synchronize()
    assert torch.equal(tok, raw[0]) and torch.equal(olen, raw[1]) and torch.equal(score.view(torch.int32), raw[2].view(torch.int32))
    tok, olen, score = tok.cpu(), olen.cpu(), score.cpu()
    for b, (rt, rs) in enumerate(ref):
        assert int(olen[b]) == len(rt) and tok[b, : len(rt)].tolist() == rt and torch.all(tok[b, len(rt):] == -1), b
        assert abs(score[b].item() - rs) <= 1e-4 * max(1.0, abs(rs)), b
    assert dec(logp.to(dev), lens.to(dev)) == [D.tokens_to_text(rt, VOCAB) for rt, _ in ref]
