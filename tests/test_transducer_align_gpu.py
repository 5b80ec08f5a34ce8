"""-m gpu: `mi355x_transducer_align` against the float32 oracle (tests/transducer_align_oracle.py) on the same `rows` -- frames,
durations and the BITS of the score are compared for equality, never with a tolerance; `mi355x_transducer_align_rows` against
float64 log-softmax; and `align` through the transducer models.  Columns per lane (nemo_amd/csrc/transducer_align.hip): 1 for
U + 1 <= 64, then 2, 4, 8, 16 up to 128, 256, 512, 1024; the next diagonal's loads are in flight for 1 and 2 only."""
import numpy as np
import pytest
import torch

import transducer_align_oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda"
DUR = {"rnnt": None, "tdt": [0, 1, 2, 3, 4], "tdt02": [0, 2], "tdt8": [0, 1, 3, 8]}


def _check(rows, act_lens, label_lens, durations):
    from nemo_amd import ops
    got = ops.transducer_align(torch.from_numpy(rows).to(dev), torch.tensor(act_lens, device=dev), torch.tensor(label_lens, device=dev),
                               durations)
    frame, dur, score = (g.cpu().numpy() for g in got)
    ref = O.align_batch(rows, act_lens, label_lens, durations)
    assert frame.dtype == dur.dtype == np.int32 and score.dtype == np.float32
    bad = np.nonzero(score.view(np.int32) != ref[2].view(np.int32))[0]
    assert bad.size == 0, (bad, score[bad], ref[2][bad])
    assert np.array_equal(frame, ref[0]) and np.array_equal(dur, ref[1])
    return frame, dur, score


def _rows(seed, B, T, U1, durations):
    return (np.random.RandomState(seed).randn(B, T, U1, 2 + len(durations or [])) - 1.0).astype(np.float32)


@pytest.mark.parametrize("U", [0, 1, 63, 64, 130, 300, 600])
@pytest.mark.parametrize("kind", sorted(DUR))
def test_lattice_is_the_oracles(kind, U):
    """T = 1, 2, 9 with U labels each: one column per lane, the 64 / 65 boundary, several columns per lane"""
    if kind == "tdt8" and U > 255:   # refused: a largest duration above 4 is served up to U + 1 = 256
        with pytest.raises(ValueError):
            _check(_rows(U, 3, 9, U + 1, DUR[kind]), [1, 2, 9], [U] * 3, DUR[kind])
        return
    _, _, score = _check(_rows(U, 3, 9, U + 1, DUR[kind]), [1, 2, 9], [U] * 3, DUR[kind])
    assert kind != "rnnt" or np.isfinite(score).all()


@pytest.mark.parametrize("kind", sorted(DUR))
def test_ragged_batch_ties_and_infinities(kind):
    act, lab = [0, 0, 9, 5, 1, 7, 9, 2, 9], [3, 0, 0, 3, 4, 70, 12, 1, 12]
    rows = _rows(7, len(act), 9, 71, DUR[kind])
    rows[6][np.random.RandomState(8).rand(*rows[6].shape) < 0.3] = -np.inf
    rows[8] = -np.inf
    frame, _, score = _check(rows, act, lab, DUR[kind])
    assert score[0] == -np.inf and (frame[0] == -1).all() and score[1] == 0.0 and score[8] == -np.inf
    # all-zero rows: every path of a lattice scores the same bits, so the path is decided by the tie rule alone
    _check(np.zeros_like(rows), act, lab, DUR[kind])


def test_duration_set_that_cannot_land():
    frame, dur, score = _check(_rows(3, 2, 6, 4, [0, 2]), [5, 6], [3, 3], [0, 2])
    assert score[0] == -np.inf and (frame[0] == -1).all() and (dur[0] == -1).all() and np.isfinite(score[1])


@pytest.mark.parametrize("V1,D", [(5, 0), (5, 5), (1025, 0), (1025, 5)])
def test_rows_kernel_against_float64(V1, D):
    """pitched logits, padded cells; tolerance = the standing one for device log-probabilities: max(8 x the float32 restatement's
    own error against float64, 16 ulp)"""
    from nemo_amd import ops
    rng = np.random.RandomState(V1 + D)
    B, T, U1, ld = 3, 3, 4, V1 + D + 3
    act, lab = [3, 2, 0], [3, 1, 2]
    acts = (4.0 * rng.randn(B, T, U1, ld)).astype(np.float32)
    labels = rng.randint(0, V1 - 1, size=(B, U1 - 1))
    rows = torch.empty(B, T, U1, 2 + D, device=dev)
    ops.transducer_align_rows(torch.from_numpy(acts).to(dev), ld, torch.from_numpy(labels).to(dev), torch.tensor(act, device=dev),
                              torch.tensor(lab, device=dev), B, T, U1, V1, D, V1 - 1, rows)
    got = rows.cpu().numpy()
    for b in range(B):
        Tb, Ub = act[b], lab[b]
        r64, r32 = (O.rows_ref(acts[b, :Tb, :Ub + 1], labels[b, :Ub], V1, D, V1 - 1, dt) for dt in (np.float64, np.float32))
        g = got[b, :Tb, :Ub + 1]
        assert np.isneginf(got[b, Tb:]).all() and np.isneginf(got[b, :, Ub + 1:]).all() and np.isneginf(g[:, Ub, 1]).all(), b
        fin = np.isfinite(r64)
        tol = np.maximum(8 * np.abs(r32[fin] - r64[fin]).max(initial=0), 16 * np.spacing(np.abs(r64[fin]).astype(np.float32)))
        err = np.abs(g[fin] - r64[fin])
        print(f"V1={V1} D={D} b={b}: max error {err.max(initial=0):.3e}, float32 restatement {np.abs(r32[fin] - r64[fin]).max(initial=0):.3e}")
        assert np.array_equal(np.isfinite(g), fin) and (err <= tol).all(), (b, err.max())


# ---------------------------------------------------------------------------------------------- through the models
VOCAB = [" "] + list("abcdefghijklmnopqrs")


def _model(kind):
    from nemo_amd import models as M
    over = dict(d_model=64, n_heads=4, n_layers=2, subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0)
    if kind == "stateless":
        over["stateless_context"] = 2
    make = {"tdt": M.fastconformer_tdt_config, "hybrid": M.fastconformer_hybrid_config}.get(kind, M.fastconformer_transducer_config)
    cfg = make("small", vocab_size=len(VOCAB), **over)
    cfg["labels"] = VOCAB
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0, **(dict(pred_rnn_layers=2) if kind == "lstm2" else {}))
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    cfg["joint"]["fused_batch_size"] = 2
    torch.manual_seed(5)
    m = (M.EncDecHybridRNNTCTCModel if kind == "hybrid" else M.EncDecRNNTModel)(cfg)
    with torch.no_grad():
        m.joint.joint_net[-1].bias[len(VOCAB)] -= 2.0   # random weights with fewer blanks: the greedy hypotheses are not empty
    return m.to(dev).eval()


def _waves():
    g = torch.Generator().manual_seed(7)
    return [0.1 * torch.randn(16000, generator=g), 0.1 * torch.randn(9600, generator=g), 0.1 * torch.randn(12000, generator=g)]


def _device_rows(model, waves, ids):
    """the aligner on the model's own encoder output, under the set-up `align` runs under -> (frame, dur, score, rows, enc_len)"""
    from nemo_amd.models.ctc_models import _audio_batch, _inference_setup
    from nemo_amd.modules import TransducerAligner
    from nemo_amd.modules.tdt_loss import TDTLoss
    tg = torch.zeros(len(ids), max(1, max(len(x) for x in ids)), dtype=torch.int64)
    for r, x in enumerate(ids):
        tg[r, :len(x)] = torch.tensor(x, dtype=torch.int64)
    durations = model.loss.durations if isinstance(model.loss, TDTLoss) else None
    with torch.no_grad(), _inference_setup(model):
        sig, lens = _audio_batch(model, waves)
        enc, n = model.forward(input_signal=sig, input_signal_length=lens)
        out = TransducerAligner(model.decoder, model.joint, durations)(enc, n, tg.to(dev), torch.tensor([len(x) for x in ids], device=dev),
                                                                       return_rows=True)
    return [t.cpu().numpy() for t in out] + [n.cpu().numpy(), durations]


@pytest.mark.parametrize("kind", ["rnnt", "tdt", "stateless", "lstm2"])
def test_model_align(kind):
    model, waves, texts = _model(kind), _waves(), ["abc", "de ", "a" * 60]   # (the last: several labels per frame)
    ids = [list(model._text_to_ids(t)) for t in texts]
    frame, dur, score, rows, n, durations = _device_rows(model, waves, ids)
    ref = O.align_batch(rows, n, [len(x) for x in ids], durations)
    aligned = model.align(waves, texts, batch_size=3)
    for r, a in enumerate(aligned):   # `align` returns the path of the float32 oracle on the rows the device produced
        k = len(ids[r]) if np.isfinite(ref[2][r]) else 0
        assert a["feasible"] == bool(np.isfinite(ref[2][r])) and np.float32(a["score"]) == ref[2][r], r
        assert [t["start_offset"] for t in a["tokens"]] == ref[0][r, :k].tolist()
        assert all(t["start_offset"] < t["end_offset"] <= max(n[r], t["start_offset"] + 1) for t in a["tokens"])
        if durations:
            assert a["token_durations"] == ref[1][r, :k].tolist()
    assert aligned[0]["feasible"] and aligned[1]["feasible"] and [w["word"] for w in aligned[0]["words"]] == ["abc"]
    # aligning the greedy transcript: Viterbi is the maximum, so not below the path through the greedy search's own frames
    hyps = model.transcribe(waves, batch_size=3, return_hypotheses=True)
    assert any(len(h.y_sequence) for h in hyps)
    _, _, score, rows, n, _ = _device_rows(model, waves, [h.y_sequence.tolist() for h in hyps])
    for r, h in enumerate(hyps):
        greedy = O.path_score(rows[r], list(h.timestamp), int(n[r]), durations)
        print(f"{kind} utterance {r}: {len(h.timestamp)} labels, viterbi {score[r]:.6f}, greedy frames {greedy:.6f}")
        assert score[r] >= greedy - 16 * np.spacing(np.abs(greedy)), (r, score[r], greedy)


def test_hybrid_default_is_the_ctc_head():
    from nemo_amd.models.ctc_models import ctc_align_audio
    model, waves, texts = _model("hybrid"), _waves()[:2], ["abc", "de"]
    assert model.align(waves, texts) == ctc_align_audio(model, waves, texts) == model.align(waves, texts, decoder_type="ctc")
    rnnt = model.align(waves, texts, decoder_type="rnnt")
    assert all(a["feasible"] for a in rnnt) and model.cur_decoder == "rnnt"
