"""-m gpu: `mi355x_ctc_align` (both kernel forms) and `mi355x_ctc_greedy_decode_ts` against the float32 oracle
(tests/ctc_align_oracle.py) -- path, first / last frames and the BITS of the score are compared for equality, never with a
tolerance -- and timestamps / forced alignment through the CTC model and the hybrid model's CTC head.

Chunk lengths, from nemo_amd/csrc/ctc.hip: the wave form stages emissions in chunks of CtcTc<P>::v = 64 (P = 1, 2), 32 (P = 4),
16 (P = 8) frames, P picked from 2*Umax+1 <= 128 / 256 / 512 / 1024; the backtrace walks chunks of CTC_BT = 64 frames in both
forms."""
import numpy as np
import pytest
import torch

import ctc_align_oracle as A

pytestmark = pytest.mark.gpu
dev = "cuda"


def _logp(rng, B, T, C):
    return torch.log_softmax(torch.from_numpy(rng.randn(B, T, C).astype(np.float32)), -1).numpy()


def _labels(rng, U, n_labels, repeats=0):
    """U labels below n_labels, no two neighbours equal except at `repeats` random places"""
    t = np.zeros(U, dtype=np.int64)
    for i in range(U):
        t[i] = rng.randint(n_labels) if i == 0 else (t[i - 1] + 1 + rng.randint(n_labels - 1)) % n_labels
    for i in rng.choice(np.arange(1, U), size=repeats, replace=False) if repeats else []:
        t[i] = t[i - 1]
    return t


def _batch(rng, cases, C, Umax=None, repeats=0):
    """cases: (T, U) or (T, target) per utterance -> (logp [B,Tmax,C], targets [B,Umax], in_len, tgt_len); blank = C - 1"""
    tg = [np.asarray(c[1], dtype=np.int64) if not np.isscalar(c[1]) else _labels(rng, c[1], C - 1, repeats) for c in cases]
    Tmax = max(1, max(c[0] for c in cases))
    Umax = Umax or max(1, max(len(t) for t in tg))
    targets = np.zeros((len(cases), Umax), dtype=np.int64)
    for b, t in enumerate(tg):
        targets[b, : len(t)] = t
    return _logp(rng, len(cases), Tmax, C), targets, np.array([c[0] for c in cases]), np.array([len(t) for t in tg])


def _check(logp, targets, in_len, tgt_len, blank, forms=(1, 0)):
    """both kernel forms against the oracle: equality of everything, the score by its bits"""
    from nemo_amd import _lib, ops
    ref = A.align_batch(logp, targets, in_len, tgt_len, blank)
    args = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (logp, targets, in_len.astype(np.int64), tgt_len.astype(np.int64))]
    for form in forms:
        prev = _lib.lib.mi355x_ctc_align_config(form)
        try:
            got = ops.ctc_align(*args, blank)
            torch.cuda.synchronize()
        finally:
            _lib.lib.mi355x_ctc_align_config(prev)
        path, ts, te, score = (g.cpu().numpy() for g in got)
        assert score.dtype == np.float32 and path.dtype == ts.dtype == te.dtype == np.int32
        bad = np.nonzero(score.view(np.int32) != ref[3].view(np.int32))[0]
        assert bad.size == 0, (form, bad, score[bad], ref[3][bad])
        assert np.array_equal(path, ref[0]), (form, np.nonzero((path != ref[0]).any(1))[0])
        assert np.array_equal(ts, ref[1]) and np.array_equal(te, ref[2]), form
    return ref


def test_align_ragged_batch_and_padding():
    rng = np.random.RandomState(0)
    cases = [(1, 1), (1, 0), (8, 0), (5, [0, 1, 2, 3, 4]),   # (5, 5) without repeats: no frame left for a blank
             (6, [3, 3, 7, 2]),    # (6, 4) with one repeat: 5 frames are needed, one is spare
             (6, [3, 3, 3, 7]),    # one label three times = two adjacent repeats: 6 frames are exactly enough
             (5, [3, 3, 3, 7]),    # ... and 5 are not
             (5, [3, 3, 7, 2]),    # one adjacent repeat: 5 frames are exactly enough
             (4, [3, 3, 7, 2]),
             (0, 0), (0, 2), (7, 3)]
    logp, targets, in_len, tgt_len = _batch(rng, cases, C=12)
    path, ts, te, score = _check(logp, targets, in_len, tgt_len, 11)
    feasible = [A.feasible_by_length(c[0], list(targets[b, : tgt_len[b]])) for b, c in enumerate(cases)]
    assert feasible == [True, True, True, True, True, True, False, True, False, True, False, True]
    assert np.array_equal(np.isfinite(score), np.array(feasible))
    assert path[3, :5].tolist() == [1, 3, 5, 7, 9] and score[9] == 0.0
    for b, c in enumerate(cases):   # the padding: -1 beyond T and beyond U, everywhere when infeasible
        assert (path[b, c[0] if feasible[b] else 0:] == -1).all() and (ts[b, tgt_len[b] if feasible[b] else 0:] == -1).all()


@pytest.mark.parametrize("U", [63, 64, 65, 127, 128, 129, 255, 256, 257, 511])
def test_align_lane_and_pair_boundaries(U):
    rng = np.random.RandomState(U)
    logp, targets, in_len, tgt_len = _batch(rng, [(U + 9, U), (U + 4, U - 2)], C=12, repeats=3)
    _, _, _, score = _check(logp, targets, in_len, tgt_len, 11)
    assert np.isfinite(score).all()


@pytest.mark.parametrize("Umax,chunk", [(63, 64), (64, 64), (200, 32), (300, 16)])   # P = 1, 2, 4, 8
def test_align_chunk_boundaries(Umax, chunk):
    """T one below, at and one above the emission chunk of the P that Umax selects, two chunks, and the backtrace chunk (64);
    U = 3 and U = T - 1"""
    rng = np.random.RandomState(chunk + Umax)
    Ts = sorted({chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 63, 64, 65, 66, 129})
    cases = [(T, 3) for T in Ts] + [(T, T - 1) for T in Ts if T - 1 <= Umax]
    logp, targets, in_len, tgt_len = _batch(rng, cases, C=12, Umax=Umax)
    _, _, _, score = _check(logp, targets, in_len, tgt_len, 11)
    assert np.isfinite(score).all()


@pytest.mark.parametrize("U,T", [(511, 530), (512, 530), (2048, 2060)])
def test_align_form_boundary_and_long_transcripts(U, T):
    """S = 1023 is the last size of the wave form, S = 1025 the first that only the LDS form takes; U = 2048 is the largest"""
    rng = np.random.RandomState(U)
    logp, targets, in_len, tgt_len = _batch(rng, [(T, U), (T - 7, U - 5)], C=8, repeats=5)
    _, _, _, score = _check(logp, targets, in_len, tgt_len, 7)
    assert np.isfinite(score).all()


def test_align_rejects_longer_transcripts():
    from nemo_amd import ops
    z = torch.zeros(1, 4, 3, device=dev)
    with pytest.raises(ValueError):
        ops.ctc_align(z, torch.zeros(1, 2049, dtype=torch.int64, device=dev), torch.tensor([4], device=dev),
                      torch.tensor([1], device=dev), 2)


def test_align_ties_are_resolved_by_rule():
    """uniform log-probabilities: every path scores the same bits, so the path is decided by the tie rule alone"""
    cases = [(9, []), (9, [4]), (9, [4, 4, 2]), (9, [1, 2, 3]), (3, [4, 4])]
    _, targets, in_len, tgt_len = _batch(np.random.RandomState(0), cases, C=6)
    logp = np.full((len(cases), 9, 6), np.float32(-1.7917595))
    path, _, _, score = _check(logp, targets, in_len, tgt_len, 5)
    assert path[0].tolist() == [0] * 9 and len(set(score[:4].tolist())) == 1
    assert path[4, :3].tolist() == [1, 2, 3]


def test_align_with_inf_emissions():
    """a random mask of -inf entries that spares one path per utterance; one utterance whose every path crosses an all -inf frame"""
    rng = np.random.RandomState(5)
    cases = [(40, 9), (33, 12), (70, 20), (25, 6), (25, 6)]
    logp, targets, in_len, tgt_len = _batch(rng, cases, C=10, Umax=70)   # (P = 2 in the wave form)
    for b, (T, U) in enumerate(cases):
        S = 2 * U + 1
        ext = np.full(S, 9)
        ext[1::2] = targets[b, :U]
        moves = np.zeros(T, dtype=np.int64)   # the spared path: from state 0 to S - 1 by S - 1 single steps at random frames
        moves[1 + rng.choice(T - 1, size=S - 1, replace=False)] = 1
        states = np.cumsum(moves)
        keep = np.zeros((T, 10), dtype=bool)
        keep[np.arange(T), ext[states]] = True
        mask = (rng.rand(T, 10) < 0.4) & ~keep
        logp[b, :T][mask] = -np.inf
    logp[4, 11, :] = -np.inf
    _, _, _, score = _check(logp, targets, in_len, tgt_len, 9)
    assert np.isfinite(score[:4]).all() and score[4] == -np.inf   # (infeasible by its emissions, not by its length)


def test_greedy_decode_with_timestamps():
    from nemo_amd import ops
    g = torch.Generator().manual_seed(41)
    T, V = 130, 28
    lens = torch.tensor([1, 63, 64, 65, 130, 130, 130, 100, 0])
    x = torch.randn(len(lens), T, V + 1, generator=g)
    x[:, :, V] += 1.5                                   # plenty of blanks
    x[1, 40:60] = x[1, 40:41]                           # a long repeat
    x[2, :, :] = torch.round(x[2] * 2) / 2              # exact ties: the first maximum wins
    x[4, 50:80, :] = x[4, 50:51, :]; x[4, 50:80, 3] += 9.0        # a run across frames 63 / 64 ...
    x[6, 60:70, :] = 0.0; x[6, 60:70, 5] = 9.0; x[6, 63, :] = 0.0; x[6, 63, 7] = 9.0   # ... and runs that end at 62, 63 and begin at 64
    x[5, :, V] += 50.0                                  # all blank
    x[7, 90:, 2] += 20.0                                # a run that reaches the last valid frame (99) and goes on in the padding
    x[3, 64, :] = 0.0; x[3, 64, 9] = 9.0; x[3, 63, V] = 9.0       # a one-frame run in the last frame of T = 65
    logp = torch.log_softmax(x, -1)
    tok0, len0, score0 = ops.ctc_greedy_decode(logp.to(dev), lens.to(dev), V)
    tok, olen, score, start, end = ops.ctc_greedy_decode_ts(logp.to(dev), lens.to(dev), V)
    torch.cuda.synchronize()
    assert torch.equal(tok, tok0) and torch.equal(olen, len0)
    assert torch.equal(score.view(torch.int32), score0.view(torch.int32))
    ref = A.greedy_ts(logp.numpy(), lens.tolist(), V)
    tok, start, end = tok.cpu(), start.cpu(), end.cpu()
    for b, (rt, rs, re_) in enumerate(ref):
        n = len(rt)
        assert int(olen[b]) == n and tok[b, :n].tolist() == rt, b
        assert start[b, :n].tolist() == rs and end[b, :n].tolist() == re_, b
        assert (start[b, n:] == -1).all() and (end[b, n:] == -1).all(), b
    assert ref[5][0] == [] and ref[8][0] == [] and ref[7][2][-1] == 99
    assert any(s <= 63 < e for s, e in zip(ref[4][1], ref[4][2]))
    # without lengths every utterance has T frames
    t2 = ops.ctc_greedy_decode_ts(logp.to(dev), None, V)
    ref2 = A.greedy_ts(logp.numpy(), None, V)
    for b, (rt, rs, re_) in enumerate(ref2):
        assert t2[3][b, : len(rt)].tolist() == rs and t2[4][b, : len(rt)].tolist() == re_


# ---------------------------------------------------------------------------------------------- through the models
VOCAB = [" "] + list("abcdefghijklmnopqrs")


def _waves():
    g = torch.Generator().manual_seed(7)
    return [0.1 * torch.randn(16000, generator=g), 0.1 * torch.randn(9600, generator=g)]


def _ctc_model():
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    torch.manual_seed(3)
    cfg = conformer_ctc_config("small", vocab_size=len(VOCAB), d_model=64, n_heads=4, n_layers=2, dropout=0.0,
                               dropout_pre_encoder=0.0, dropout_att=0.0)
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["vocabulary"] = VOCAB
    cfg["labels"] = VOCAB
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


@pytest.mark.parametrize("kind", ["ctc", "hybrid"])
def test_model_timestamps_and_alignment(kind):
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    model = _ctc_model() if kind == "ctc" else _hybrid_model()
    waves = _waves()
    if kind == "hybrid":
        aligned_rnnt = model.align(waves, ["abc", "de"])      # the CTC head aligns whichever head decodes
        assert model.cur_decoder == "rnnt" and all(a["feasible"] for a in aligned_rnnt)
        with pytest.raises(NotImplementedError):
            model.transcribe(waves, timestamps=True)
        model.change_decoding_strategy(decoder_type="ctc")
    texts = model.transcribe(waves, batch_size=2)
    hyps = model.transcribe(waves, batch_size=2, timestamps=True)
    stride = model.frame_stride_s
    assert [h.text for h in hyps] == texts and any(len(h.y_sequence) for h in hyps)
    for h in hyps:
        ts = h.timestamp
        assert [VOCAB.index(c["char"]) for c in ts["char"]] == h.y_sequence.tolist()
        assert ts["timestep"] == [c["start_offset"] for c in ts["char"]] and ts["timestep"] == sorted(ts["timestep"])
        for o in ts["char"] + ts["word"]:
            assert o["start_offset"] < o["end_offset"] <= h.length
            assert o["start"] == o["start_offset"] * stride and o["end"] == o["end_offset"] * stride
        assert " ".join(w["word"] for w in ts["word"]) == " ".join(h.text.split())
    # align(audio, transcribe(audio)): feasible, and at least as probable as the greedy path (blank frames included)
    # (the log-probabilities as `align` computes them: the same batch under the same set-up, so both sums add the same numbers)
    with torch.no_grad(), _inference_setup(model):
        lp, n = model._ctc_log_probs(*_audio_batch(model, waves))
    aligned = model.align(waves, texts, batch_size=2)
    for r, a in enumerate(aligned):
        T = int(n[r])
        greedy_total = A.path_score(lp[r, :T].max(-1).values.cpu().numpy()[:, None], [0] * T, [], 0)   # f32, frame by frame
        assert a["feasible"] and len(a["tokens"]) == len(hyps[r].y_sequence)
        # (the greedy path is one alignment of its own transcript, summed in float32 in the order the recursion adds)
        assert np.float32(a["score"]) >= greedy_total, (a["score"], greedy_total)
        starts = [t["start_offset"] for t in a["tokens"]]
        assert starts == sorted(starts) and all(t["start"] == t["start_offset"] * stride for t in a["tokens"])
        assert all(t["end_offset"] <= T for t in a["tokens"])
    # more labels than frames: flagged, not raised
    long = model.align(waves[1:], ["ab" * 100])
    assert long[0]["feasible"] is False and long[0]["score"] == float("-inf") and long[0]["tokens"] == [] and long[0]["words"] == []
