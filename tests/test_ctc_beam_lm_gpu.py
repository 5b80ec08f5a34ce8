"""-m gpu: `mi355x_ctc_beam_decode_lm` against the float64 oracle of the search with n-gram fusion (tests/ctc_beam_lm_oracle.py), and
`beam.ngram_lm_arpa` through the decoding object, the CTC model and the hybrid model's CTC head.

Parity rule, the one of test_ctc_beam_gpu.py: a (shape, seed) case is compared only if the float64 oracle's cut margin -- min over
the frames of rank[W-1] - rank[W] -- is >= 1e-3 (a condition on the input, not a measurement of the device).  Seeds 0..23 of
`O.make_logp` are taken per shape with the model `make_lm(0, C-1, order)`, and at least 5 must pass the rule, else the test FAILS.
Kept by the oracle on a CPU: 23, 20, 22, 15, 17, 12, 8 seeds for the seven shapes; on every kept case the float32 restatement of the
oracle keeps the float64 set of hypotheses and differs from it by <= 1.1e-4, and the n-best differs from the LM-less oracle's, so
no case passes by ignoring the LM (asserted below).

In a kept case: the device's set of hypotheses equals the oracle's, n_hyp and hyp_len are equal, device scores are non-increasing,
each score is within max(8 * e32, 16 ulp of the score) of float64 where e32 is the float32 restatement's own largest error on that
case (reference against reference, never the device), every tok_frame is strictly increasing along its hypothesis and lies in
[0, len), and the -1 / -inf padding is exact."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_lm_oracle as L
import ctc_beam_oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda"
INF = float("inf")
MARGIN = 1e-3
VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]

# (T, C, W, threshold, beta, alpha, order); blank = C - 1
SHAPES = [
    (37, 5, 4, INF, 0.0, 0.5, 3),       # C < 64: every look-up in one group of classes
    (70, 29, 8, INF, 0.0, 0.3, 3),      # crossing 64 frames
    (200, 33, 3, INF, 0.0, 0.5, 2),     # W not a power of two, long chase, bigram model
    (24, 129, 16, 8.0, 0.5, 0.5, 4),    # three groups of 64 classes, finite threshold, beta, 4-gram: the longest back-off chains
    (66, 129, 8, 8.0, 0.5, 1.0, 2),     # alpha = 1 with beta
    (24, 70, 64, INF, 0.0, 0.5, 3),     # full wave, no pruning
    (12, 1025, 64, 6.0, 0.0, 0.3, 3),   # full wave, BPE width: >= 189 candidates for the 64 places in every frame
]


@functools.lru_cache(maxsize=None)
def _model(V, order):
    return L.make_lm(0, V, order)


@functools.lru_cache(maxsize=None)
def _device_lm(V, order):
    """the model through the product's own path: ARPA text -> NGramLM"""
    import os
    import tempfile
    from nemo_amd.modules import NGramLM
    with tempfile.TemporaryDirectory() as d:
        L.write_arpa(_model(V, order), os.path.join(d, "lm.arpa"))
        return NGramLM.from_arpa(os.path.join(d, "lm.arpa"), V)


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


@functools.lru_cache(maxsize=None)
def _reference(seed, T, C, W, theta, beta, alpha, order):
    """(logp, float64 result, float32 result or None) of one utterance; the float32 run only where the case is kept"""
    lp = O.make_logp(seed, T, C)
    ng = _model(C - 1, order)
    r64 = L.beam_search_lm(lp, C - 1, W, theta, beta, alpha, ng, order)
    r32 = L.beam_search_lm(lp, C - 1, W, theta, beta, alpha, ng, order, dtype=np.float32) if r64["margin"] >= MARGIN else None
    return lp, r64, r32


def _e32(r64, r32):
    d64 = dict(r64["nbest"])
    common = [abs(float(s) - float(d64[p])) for p, s in r32["nbest"] if p in d64]
    return max(common) if common else 0.0


def _decode(logp, lens, W, theta, beta, alpha, order, lm=None):
    from nemo_amd import ops
    lp = torch.from_numpy(np.ascontiguousarray(logp)).to(dev)
    ln = torch.tensor(lens, dtype=torch.int64, device=dev)
    C = logp.shape[2]
    if order is None:
        out = ops.ctc_beam_decode(lp, ln, C - 1, W, theta, beta)
    else:
        out = ops.ctc_beam_decode_lm(lp, ln, C - 1, W, theta, beta, lm or _device_lm(C - 1, order), alpha)
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


@pytest.mark.parametrize("T,C,W,theta,beta,alpha,order", SHAPES)
def test_fused_beam_search_matches_the_oracle(T, C, W, theta, beta, alpha, order):
    shape = (T, C, W, theta, beta, alpha, order)
    kept = [s for s in range(24) if _reference(s, *shape)[2] is not None]
    print(f"CTC_BEAM_LM kept {shape}: {len(kept)} of 24 seeds {kept}")
    assert len(kept) >= 5, kept
    refs = [_reference(s, *shape) for s in kept]
    if C == 1025:
        assert all(r64["min_candidates"] >= 189 for _, r64, _ in refs), [r64["min_candidates"] for _, r64, _ in refs]
    for lp, r64, r32 in refs:   # conditions on the references: the float32 restatement keeps the set, and the LM matters
        assert set(p for p, _ in r32["nbest"]) == set(p for p, _ in r64["nbest"]) and _e32(r64, r32) <= 1.1e-4
        assert [p for p, _ in O.beam_search(lp, C - 1, W, theta, beta)["nbest"]] != [p for p, _ in r64["nbest"]]
    logp = np.stack([lp for lp, _, _ in refs])
    out = _decode(logp, [T] * len(kept), W, theta, beta, alpha, order)
    worst = (0.0, 0.0)
    for b, (seed, (_, r64, r32)) in enumerate(zip(kept, refs)):
        w = _check_row(shape + (seed,), T, W, *(o[b] for o in out), dict(r64["nbest"]), _e32(r64, r32))
        if w[0] / max(w[1], 1e-300) >= worst[0] / max(worst[1], 1e-300):
            worst = w
    print(f"CTC_BEAM_LM err {shape}: largest score error {worst[0]:.3e} against its bound {worst[1]:.3e}")


@pytest.mark.parametrize("T,C,W,theta,beta,alpha,order", [SHAPES[3], SHAPES[5]])
def test_alpha_zero_gives_the_bits_of_the_lm_less_entry(T, C, W, theta, beta, alpha, order):
    logp = np.stack([O.make_logp(s, T, C) for s in range(6)])
    lens = [T, T - 1, T, 3, T, T // 2]
    plain = _decode(logp, lens, W, theta, beta, None, None)
    fused = _decode(logp, lens, W, theta, beta, 0.0, order)
    for name, a, b in zip(("tokens", "tok_frame", "hyp_len", "score", "n_hyp"), plain, fused):
        assert a.tobytes() == b.tobytes(), name
    assert _decode(logp, lens, W, theta, beta, alpha, order)[3].tobytes() != plain[3].tobytes()   # (and alpha > 0 is another search)


def _first_kept(T, C, W, alpha, order, start=0):
    for s in range(start, start + 64):
        if _reference(s, T, C, W, INF, 0.0, alpha, order)[2] is not None:
            return s
    raise AssertionError("no seed passes the cut-margin rule")


def test_ragged_batch_junk_beyond_the_lengths_and_the_exhaustive_case():
    """one batch, C = 3, W = 64: lengths {11, 10, 1, 0, 4} with NaN beyond each length; the length-0 row is one empty hypothesis with
    score 0 and the length-4 row all 15 prefixes, each scored ctc_loglik + alpha * lm exactly (no margin needed)"""
    T, C, W, alpha, order = 11, 3, 64, 0.5, 3
    lens = [T, T - 1, 1, 0, 4]
    seeds = [_first_kept(T, C, W, alpha, order), _first_kept(T - 1, C, W, alpha, order, 100), 7, 0, 3]
    logp = np.full((len(lens), T, C), np.nan, dtype=np.float32)
    refs = []
    for b, (n, s) in enumerate(zip(lens, seeds)):
        if n:
            lp, r64, r32 = _reference(s, n, C, W, INF, 0.0, alpha, order)
            logp[b, :n] = lp
        else:
            r64 = r32 = dict(nbest=[((), 0.0)], margin=np.inf, min_candidates=0)
        assert r32 is not None
        refs.append((r64, r32))
    out = _decode(logp, lens, W, INF, 0.0, alpha, order)
    for b, (r64, r32) in enumerate(refs):
        err, tol = _check_row(("ragged", b), lens[b], W, *(o[b] for o in out), dict(r64["nbest"]), _e32(r64, r32))
        print(f"CTC_BEAM_LM ragged row {b} len={lens[b]}: n_hyp={out[4][b]} err={err:.3e} tol={tol:.3e}")
    assert out[4].tolist()[2:] == [3, 1, 15]
    assert out[3][3, 0] == 0.0 and out[2][3, 0] == 0
    lp4, r64, r32 = _reference(3, 4, C, W, INF, 0.0, alpha, order)
    ng = _model(C - 1, order)
    exact = {p: O.ctc_loglik(lp4, list(p), C - 1) + alpha * L.lm_score(ng, order, p) for p, _ in r64["nbest"]}
    assert len(exact) == 15
    _check_row("exhaustive", 4, W, *(o[4] for o in out), exact, _e32(r64, r32))


def test_the_lm_flips_a_hand_written_case(tmp_path):
    """T = 2, C = 4 (a, b, c, blank).  Frame 0 says a; frame 1 prefers b over c by 0.2; the LM prefers c behind a by 2.0 (and gives
    c behind a a high probability, so that `a c` also stays ahead of the shorter `a`).  alpha = 0: `a b`; alpha = 1: `a c`."""
    from nemo_amd.modules import NGramLM
    p1b = 0.45
    p = np.array([[0.90, 0.03, 0.03, 0.04], [0.08, p1b, p1b * np.exp(-0.2), 1.0 - 0.08 - p1b - p1b * np.exp(-0.2)]])
    lp = np.log(p).astype(np.float32)
    ng = {(0,): [-1.0, -0.3], (1,): [-1.0, -0.3], (2,): [-1.0, -0.3], (L.BOS,): [-99.0, -0.2],
          (0, 2): [-0.05, 0.0], (0, 1): [-0.05 - 2.0 / L.LN10, 0.0]}
    L.write_arpa(ng, tmp_path / "flip.arpa")
    lm = NGramLM.from_arpa(tmp_path / "flip.arpa", 3)
    assert abs((lm.score([0, 2]) - lm.score([0, 1])) - 2.0) < 1e-5
    for alpha, best in ((0.0, (0, 1)), (1.0, (0, 2))):
        r64 = L.beam_search_lm(lp, 3, 8, INF, 0.0, alpha, ng, 2)
        r32 = L.beam_search_lm(lp, 3, 8, INF, 0.0, alpha, ng, 2, dtype=np.float32)
        assert r64["nbest"][0][0] == best and r64["nbest"][0][1] - r64["nbest"][1][1] > 0.1
        out = _decode(lp[None], [2], 8, INF, 0.0, alpha, 2, lm=lm)
        assert tuple(out[0][0, 0, : out[2][0, 0]].tolist()) == best
        _check_row(("flip", alpha), 2, 8, *(o[0] for o in out), dict(r64["nbest"]), _e32(r64, r32))


def test_bad_arguments_raise():
    from nemo_amd import ops
    lp = torch.zeros(1, 4, 5, device=dev)
    lens = torch.tensor([4], device=dev)
    lm = _device_lm(4, 3)
    args = dict(blank=4, beam_size=4, beam_threshold=20.0, beam_beta=0.0, lm=lm, alpha=0.5)
    for kw in (dict(alpha=-0.5), dict(alpha=float("nan")), dict(blank=3), dict(beam_size=65), dict(lm=_device_lm(28, 3))):
        with pytest.raises(ValueError):
            ops.ctc_beam_decode_lm(lp, lens, **dict(args, **kw))
    with pytest.raises(TypeError):
        ops.ctc_beam_decode_lm(lp, lens, **dict(args, lm=lm.to(dev)))   # loose tensors are not taken


# ---------------------------------------------------------------------------------------------- decoding object and models
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


def _check_model(model, waves, with_lm):
    """transcribe under beam_batch = the decoding object on the model's own log-probabilities"""
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    dec = model._ctc_decoding()
    assert type(dec).__name__ == "BeamBatchedCTCDecoder" and dec.beam_size == 4 and not dec.return_best_hypothesis
    assert (dec.ngram_lm is not None and dec.ngram_lm.vocab_size == len(VOCAB) and dec.ngram_lm_alpha == 0.7) if with_lm else dec.ngram_lm is None
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
    with pytest.raises(NotImplementedError, match="timestamps"):
        model.transcribe(waves, timestamps=True)
    if with_lm:   # score = acoustic part + alpha * lm, and the acoustic part is what the search kept of the sequence's alignments, so
        # the exact likelihood bounds it (what is subtracted is mostly several units per token: a score without it would not pass).
        # Slack for float32: <= 32 frames here, 4 roundings a frame, ulp(256) = 3.1e-5 each: 3.9e-3
        lp_cpu, n_cpu = lp.float().cpu().numpy(), n.cpu().tolist()
        assert max(n_cpu) <= 32
        for b, w in enumerate(want):
            for ids, s in w:
                am = s - dec.ngram_lm_alpha * dec.ngram_lm.score(ids)
                assert abs(s) < 256 and am <= O.ctc_loglik(lp_cpu[b, : n_cpu[b]], ids, len(VOCAB)) + 3.9e-3, (b, ids)
    return lists


def _predict_best(model):
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    with torch.no_grad(), _inference_setup(model):
        sig, lens = _audio_batch(model, _waves())
        return [t for _, t in model.predict_step((sig, lens, None, None, [0, 1]))]


BEAM4 = dict(strategy="beam_batch", beam=dict(beam_size=4, return_best_hypothesis=False))


def _beam4_lm(tmp_path):
    L.write_arpa(_model(len(VOCAB), 3), tmp_path / "chars.arpa")
    return dict(strategy="beam_batch", beam=dict(beam_size=4, return_best_hypothesis=False, ngram_lm_arpa=str(tmp_path / "chars.arpa"),
                                                 ngram_lm_alpha=0.7))


def test_ctc_model_transcribes_with_the_fused_search(tmp_path):
    model = _ctc_model(_beam4_lm(tmp_path))
    lists = _check_model(model, _waves(), True)
    assert _predict_best(model) == [l[0][0] for l in lists]   # predict_step scores the best hypothesis
    plain = _check_model(_ctc_model(BEAM4), _waves(), False)
    assert [[(ids, s) for _, ids, s in l] for l in lists] != [[(ids, s) for _, ids, s in l] for l in plain]


def test_hybrid_ctc_head_transcribes_with_the_fused_search(tmp_path):
    model = _hybrid_model()
    model.change_decoding_strategy(BEAM4, decoder_type="ctc")
    plain = _check_model(model, _waves(), False)
    model.change_decoding_strategy(_beam4_lm(tmp_path), decoder_type="ctc")
    lists = _check_model(model, _waves(), True)
    assert _predict_best(model) == [l[0][0] for l in lists]
    assert [[(ids, s) for _, ids, s in l] for l in lists] != [[(ids, s) for _, ids, s in l] for l in plain]
