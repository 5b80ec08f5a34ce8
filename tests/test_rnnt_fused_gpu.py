"""-m gpu: the greedy transducer search with shallow fusion (mi355x_transducer_greedy_decode_fused, csrc/rnnt_decode.hip: the NM > 0
instantiations of the greedy kernel) against the float64 restatement (tests/rnnt_fused_oracle.py), and `fusion_models` through the
decoding objects and the models.

  1. parity: the device's hypotheses walked through the restatement's forced walk, by the project's rule for this kind of check
     (tests/test_rnnt_decoding.py, `_rule2` of tests/test_stream_decode_gpu.py): a decision taken differently has a margin
     <= 2e-4 x the step's largest |logit|, and at most 2 % of the decisions differ;
  2. score: against the float64 score of the device's own hypothesis, final terms included, within max(8 x e32, 16 ulp), e32 = the
     float32 restatement's distance from the float64 one on that hypothesis (the bound of tests/test_confidence_gpu.py);
  3. every alpha = 0: the bits of ops.rnnt_greedy_decode / ops.tdt_greedy_decode;
  4. any cut into chunks: the bits of one launch, every field of the state included.
The input conditions of the cases (labels, decisions the models change, pending and completed phrases) are asserted on the CPU by
tests/test_rnnt_fused_host.py."""
import numpy as np
import pytest
import torch

import rnnt_fused_oracle as R
import stream_decode_oracle as S
from test_stream_decode_gpu import _bf16_images, _dev_args

pytestmark = pytest.mark.gpu
dev = "cuda"
MS = R.MAX_SYMBOLS


def _rule(rows_per_utt, n_labels, min_labels):
    """the two rules of `_rule2` (its counts are the recipe geometry's; here the case's own, asserted on the CPU beforehand)"""
    decisions = [r for rows in rows_per_utt for r in rows]
    flips = [r for r in decisions if r[1] != r[2]]
    assert n_labels > min_labels and len(decisions) > n_labels, (len(decisions), n_labels)
    for t, follow, own, margin, scale in flips:
        assert margin <= 2e-4 * scale, (t, follow, own, margin, scale)
    assert len(flips) <= 0.02 * len(decisions), (len(flips), len(decisions))
    return len(flips), len(decisions)


def _fused(ops, f, lens, args, V, pairs, durations, state=None):
    return ops.transducer_greedy_decode_fused(f, lens, *args, V, MS, pairs, durations=durations, state=state)


def _hyps(tk, tm, n):
    tk, tm, n = tk.cpu(), tm.cpu(), n.cpu()
    for b in range(tk.shape[0]):
        assert (tk[b, int(n[b]):] == -1).all() and (tm[b, int(n[b]):] == -1).all()
    return [(tk[b, : int(n[b])].tolist(), tm[b, : int(n[b])].tolist()) for b in range(tk.shape[0])]


def _check_against_oracle(case, which, hyps, score, P64, f64, P32, f32, min_labels):
    """rule 1 and the score bound for the device's hypotheses `hyps` / scores; P64 / P32 = (Pd, Pj) in float64 / float32"""
    models, _ = R.case_models(case, which)
    rep, sc64 = R.forced_walk(*P64, f64, case["lens"], case["V"], MS, models, hyps, case["durations"])
    n_labels = sum(len(h[0]) for h in hyps)
    print(which, "flips / decisions:", _rule(rep, n_labels, min_labels))
    _, sc32 = R.forced_walk(*P32, f32, case["lens"], case["V"], MS, models, hyps, case["durations"])
    got = score.cpu().numpy()
    for b, (a64, a32) in enumerate(zip(sc64, sc32)):
        e32 = abs(float(a32) - float(a64))
        tol = max(8 * e32, 16 * float(np.spacing(np.float32(abs(a64)))))
        print(f"  utt {b}: score {got[b]!r} float64 {a64!r} |device - float64| {abs(float(got[b]) - a64):.3e} e32 {e32:.3e} tol {tol:.3e}")
    for b, (a64, a32) in enumerate(zip(sc64, sc32)):
        e32 = abs(float(a32) - float(a64))
        assert abs(float(got[b]) - float(a64)) <= max(8 * e32, 16 * float(np.spacing(np.float32(abs(a64))))), b


@pytest.mark.parametrize("which", ["tree", "lm", "both"])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_fused_search_against_the_float64_restatement(kind, which):
    from nemo_amd import ops
    case = R.fused_case(kind)
    _, pairs = R.case_models(case, which)
    args = _dev_args(case["Pd"], case["Pj"], torch.float32)
    tk, tm, n, score, (h, c) = _fused(ops, case["f_all"].to(dev), case["lens"].to(dev), args, case["V"], pairs, case["durations"])
    hyps = _hyps(tk, tm, n)
    assert hyps != case["base"]   # the models changed the search
    _check_against_oracle(case, which, hyps, score, (case["Pd64"], case["Pj64"]), case["f_all"].double(),
                          (case["Pd"], case["Pj"]), case["f_all"], 40)


@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_fused_search_over_a_wide_vocabulary(kind):
    """V1 = 1101: three strides of the 512-thread ranking pass, the last one partial"""
    from nemo_amd import ops
    case = R.fused_case(kind, "wide")
    _, pairs = R.case_models(case, "both")
    args = _dev_args(case["Pd"], case["Pj"], torch.float32)
    tk, tm, n, score, _ = _fused(ops, case["f_all"].to(dev), case["lens"].to(dev), args, case["V"], pairs, case["durations"])
    hyps = _hyps(tk, tm, n)
    assert hyps != case["base"]
    _check_against_oracle(case, "both", hyps, score, (case["Pd64"], case["Pj64"]), case["f_all"].double(),
                          (case["Pd"], case["Pj"]), case["f_all"], 20)


@pytest.mark.parametrize("kind,which", [("rnnt", "tree"), ("tdt", "lm")])
def test_fused_search_with_bf16_weight_images(kind, which):
    """the forced walk over bf16-rounded weights and projection (`_bf16_images` of tests/test_stream_decode_gpu.py)"""
    from nemo_amd import ops
    case = R.fused_case(kind)
    _, pairs = R.case_models(case, which)
    Pd16, Pj16, f16 = _bf16_images(case["Pd"], case["Pj"], case["enc"])
    args16 = _dev_args(case["Pd"], case["Pj"], torch.bfloat16)
    tk, tm, n, score, _ = _fused(ops, f16.to(dev).to(torch.bfloat16), case["lens"].to(dev), args16, case["V"], pairs, case["durations"])
    hyps = _hyps(tk, tm, n)
    models, _ = R.case_models(case, which)
    rep, _ = R.forced_walk(R.to64(Pd16), R.to64(Pj16), f16.double(), case["lens"], case["V"], MS, models, hyps, case["durations"])
    print("bf16 flips / decisions:", _rule(rep, sum(len(h[0]) for h in hyps), 40))


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_zero_weights_give_the_bits_of_the_unfused_search(kind, wdt):
    from nemo_amd import ops
    case = R.fused_case(kind)
    _, pairs = R.case_models(case, "both", tree_alpha=0.0, lm_alpha=0.0)
    assert [a for _, a in pairs] == [0.0, 0.0]
    args = _dev_args(case["Pd"], case["Pj"], wdt)
    f, lens, V = case["f_all"].to(dev).to(wdt), case["lens"].to(dev), case["V"]
    got = _fused(ops, f, lens, args, V, pairs, case["durations"])
    if kind == "rnnt":
        want = ops.rnnt_greedy_decode(f, lens, *args, V, MS, with_state=True)
    else:
        want = ops.tdt_greedy_decode(f, lens, *args, V, R.DUR, MS, with_state=True)
    assert int(want[2].sum()) > 40
    for name, a, b in zip(("tokens", "frames", "lengths", "score"), got[:4], want[:4]):
        assert torch.equal(a, b), name
    assert torch.equal(got[4][0], want[4][0]) and torch.equal(got[4][1], want[4][1])
    # and through the resumable form: the state of the unfused resumable search
    st = ops.RNNTFusedStreamState.fresh(f.shape[0], args[0].shape[1], V, dev)
    tk, tm, n, sc, nxt = _fused(ops, f, lens, args, V, pairs, case["durations"], state=st)
    if kind == "rnnt":
        wtk, wtm, wn, wst = ops.rnnt_greedy_decode_stream(f, lens, *args, V, MS)
    else:
        wtk, wtm, wn, wst = ops.tdt_greedy_decode_stream(f, lens, *args, V, R.DUR, MS)
    assert torch.equal(tk, wtk) and torch.equal(tm, wtm) and torch.equal(n, wn) and torch.equal(sc, wst.score)
    for a in ("h", "c", "last", "score", "frames_done", "skip", "zero_run"):
        assert torch.equal(getattr(nxt, a), getattr(wst, a)), a


def _run_chunked(ops, f_all, lens, args, V, pairs, durations, edges):
    B = f_all.shape[0]
    toks, times = [[] for _ in range(B)], [[] for _ in range(B)]
    state = ops.RNNTFusedStreamState.fresh(B, args[0].shape[1], V, dev)
    score = None
    for lo, hi in zip(edges[:-1], edges[1:]):
        cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
        fc = f_all[:, lo:hi].contiguous()
        tk, tm, n, score, nxt = _fused(ops, fc, cl, args, V, pairs, durations, state=state)
        again = _fused(ops, fc, cl, args, V, pairs, durations, state=state)   # the same state_in stepped twice: the same result
        assert all(torch.equal(a, b) for a, b in zip((tk, tm, n, score) + nxt.tensors(), again[:4] + again[4].tensors()))
        for b, (t_b, f_b) in enumerate(_hyps(tk, tm, n)):
            toks[b] += t_b; times[b] += f_b
        state = nxt
    return list(zip(toks, times)), score, state


@pytest.mark.parametrize("which", ["tree", "both"])
@pytest.mark.parametrize("kind", ["rnnt", "tdt"])
def test_chunked_fused_search_equals_one_launch_bit_for_bit(kind, which):
    from nemo_amd import ops
    case = R.fused_case(kind)
    _, pairs = R.case_models(case, which)
    T, V = S.SMALL["T"], case["V"]
    lens = torch.tensor([37, 30, 0, 9])   # ragged, one stream without a frame
    args = _dev_args(case["Pd"], case["Pj"], torch.float32)
    f_all = case["f_all"].to(dev)
    one, sc1, st1 = _run_chunked(ops, f_all, lens, args, V, pairs, case["durations"], [0, T])
    # the one-shot call (no states) is that launch
    tk, tm, n, sc, (h, c) = _fused(ops, f_all, lens.to(dev), args, V, pairs, case["durations"])
    assert _hyps(tk, tm, n) == one and torch.equal(sc, sc1) and torch.equal(h, st1.h) and torch.equal(c, st1.c)
    assert sum(len(o[0]) for o in one) > 40 and one[2] == ([], [])
    assert not torch.equal(sc1, st1.score)   # a phrase was pending at the end: the output took its boost back, the state did not
    assert bool((st1.m_state[:, : len(pairs)] != 1).any())
    g = torch.Generator().manual_seed(78)
    rnd = sorted(set(torch.randint(1, T, (5,), generator=g).tolist()))
    for edges in ([0, T], list(range(T + 1)), [0, 1, 14, 27, T], [0] + rnd + [T]):
        got, sc, st = _run_chunked(ops, f_all, lens, args, V, pairs, case["durations"], edges)
        assert got == one and torch.equal(sc, sc1), edges
        for a in ("h", "c", "last", "score", "frames_done", "skip", "zero_run", "m_state"):
            assert torch.equal(getattr(st, a), getattr(st1, a)), (edges, a)


def test_tdt_decoder_object_resumes_fused_streams():
    """GreedyBatchedTDTInfer(fusion_models=...): forward with partial_hypotheses over chunks of the whole-sequence projection
    equals the one-shot forward in y_sequence, timestamp and score; token confidence together with fusion is refused.
    `infer._project` is replaced, so the encoder chunks passed in are not read: this shows that `forward` carries state and score
    through, not that a per-chunk projection GEMM gives the whole-sequence one's bits (the op-level chunking test above covers the
    kernel; tests/test_stream_decode_gpu.py the projection of the plain decoder objects)"""
    from nemo_amd import ops
    from nemo_amd.modules import GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTDecoder, RNNTJoint
    case = R.fused_case("tdt")
    _, pairs = R.case_models(case, "both")
    V, H, D, J, T = (S.SMALL[k] for k in "VHDJT")
    dec = RNNTDecoder(prednet={"pred_hidden": H, "pred_rnn_layers": 1, "dropout": 0.0}, vocab_size=V, compute_dtype=torch.float32)
    joint = RNNTJoint(jointnet={"encoder_hidden": D, "pred_hidden": H, "joint_hidden": J, "activation": "relu", "dropout": 0.0},
                      num_classes=V, num_extra_outputs=len(R.DUR), compute_dtype=torch.float32)
    out = [k[:-len("weight")] for k in joint.state_dict() if k.startswith("joint_net.") and k.endswith(".weight")][0]
    dec.load_state_dict(case["Pd"]); joint.load_state_dict({k.replace("joint_net.2.", out): v for k, v in case["Pj"].items()})
    dec, joint = dec.to(dev).eval(), joint.to(dev).eval()
    with pytest.raises(NotImplementedError, match="fusion_models.*confidence_cfg"):
        GreedyBatchedRNNTInfer(dec, joint, V, max_symbols_per_step=MS, fusion_models=pairs,
                               confidence_cfg={"preserve_token_confidence": True})
    infer = GreedyBatchedTDTInfer(dec, joint, V, R.DUR, max_symbols_per_step=MS, fusion_models=pairs)
    plain = GreedyBatchedTDTInfer(dec, joint, V, R.DUR, max_symbols_per_step=MS)
    encd, lens = case["enc"].to(dev), case["lens"]
    whole = infer(encoder_output=encd, encoded_lengths=lens.to(dev))[0]
    assert [w.y_sequence.tolist() for w in whole] != [w.y_sequence.tolist() for w in plain(encoder_output=encd, encoded_lengths=lens.to(dev))[0]]
    f_whole, args = infer._project(encd)
    hyps = infer.fresh_hypotheses(len(lens))
    assert all(isinstance(h.dec_state, ops.RNNTFusedStreamState) for h in hyps)
    project = infer._project
    try:
        for lo, hi in zip([0, 13, 26], [13, 26, T]):
            infer._project = lambda chunk, lo=lo, hi=hi: (f_whole[:, lo:hi].contiguous(), args)
            cl = (lens - lo).clamp(min=0, max=hi - lo).to(dev)
            hyps = infer(encoder_output=encd[:, :, lo:hi].contiguous(), encoded_lengths=cl, partial_hypotheses=hyps)[0]
    finally:
        infer._project = project
    assert sum(len(w.y_sequence) for w in whole) > 40
    for b, (h, w) in enumerate(zip(hyps, whole)):
        assert h.y_sequence.tolist() == w.y_sequence.tolist() and h.timestamp == w.timestamp and h.score == w.score, b
        assert h.length == w.length


VOCAB = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


def _model_cfg(hybrid, greedy):
    from nemo_amd.models import fastconformer_hybrid_config, fastconformer_transducer_config
    over = dict(d_model=64, n_heads=4, n_layers=2, subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0,
                compute_dtype=torch.float32)
    cfg = (fastconformer_hybrid_config("small", vocab_size=len(VOCAB), ctc_loss_weight=0.3, **over) if hybrid else
           fastconformer_transducer_config("small", vocab_size=len(VOCAB), **over))
    cfg["labels"] = VOCAB
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    cfg["decoding"] = dict(strategy="greedy_batch", greedy=dict(greedy, max_symbols=3))
    return cfg


@pytest.mark.parametrize("hybrid", [False, True])
def test_models_transcribe_through_the_fused_search(hybrid, monkeypatch):
    from nemo_amd import ops
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel
    from nemo_amd.modules.boosting_tree import BoostingTree
    cls = EncDecHybridRNNTCTCModel if hybrid else EncDecRNNTModel

    def build(greedy):
        torch.manual_seed(4)
        m = cls(_model_cfg(hybrid, greedy))
        with torch.no_grad():   # a transducer head that emits labels
            for p in list(m.decoder.parameters()) + list(m.joint.parameters()):
                p.mul_(4.0)
        return m.to(dev).eval()

    g = torch.Generator().manual_seed(7)
    waves = [0.1 * torch.randn(32000, generator=g), 0.1 * torch.randn(19200, generator=g)]
    before = build({}).transcribe(waves, batch_size=2, return_hypotheses=True)
    ids = [h.y_sequence.tolist() for h in before]
    print("labels of the plain search:", [len(i) for i in ids])
    assert sum(len(i) for i in ids) >= 12
    # phrases the plain search begins and does not finish: two of its own labels, then another letter
    phrases = ["".join(VOCAB[j] for j in i[k:k + 2]) + VOCAB[(i[k + 2] + 1 + k) % 26] for i in ids for k in range(0, len(i) - 2, 2)]
    phrases = sorted({p for p in phrases if p.isalpha()})
    assert len(phrases) >= 3
    greedy = dict(boosting_tree=dict(key_phrases_list=phrases, context_score=1.0, depth_scaling=2.0), boosting_tree_alpha=4.0)
    m = build(greedy)
    calls = []
    real = ops.transducer_greedy_decode_fused
    monkeypatch.setattr(ops, "transducer_greedy_decode_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    hyps = m.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert calls and [h.y_sequence.tolist() for h in hyps] != ids
    # the ids of a direct call of the op on the same encoder output
    sig = torch.zeros(2, 32000)
    for r, w in enumerate(waves):
        sig[r, : w.numel()] = w
    with torch.no_grad():
        enc, enc_len = m.forward(input_signal=sig.to(dev), input_signal_length=torch.tensor([32000, 19200]).to(dev))
    infer = m.decoding.decoding
    assert len(infer.fusion_models) == 1 and isinstance(infer.fusion_models[0][0], BoostingTree) and infer.fusion_models[0][1] == 4.0
    f, args = infer._project(enc)
    tree = BoostingTree.from_phrases([[VOCAB.index(ch) for ch in p] for p in phrases], len(VOCAB))
    tk, tm, n, sc, _ = real(f, enc_len.to(torch.int64), *args, [(tree, 4.0)])
    direct = _hyps(tk, tm, n)
    via = m.decoding.rnnt_decoder_predictions_tensor(enc, enc_len)
    assert [(h.y_sequence.tolist(), h.timestamp) for h in via] == direct
    assert [h.y_sequence.tolist() for h in hyps] == [d[0] for d in direct] and [h.score for h in via] == sc.tolist()
    # back to a section without the keys: the search it was
    n_calls = len(calls)
    if hybrid:
        m.change_decoding_strategy(dict(strategy="greedy_batch", greedy=dict(max_symbols=3)), decoder_type="rnnt")
    else:
        m.change_decoding_strategy(dict(strategy="greedy_batch", greedy=dict(max_symbols=3)))
    after = m.transcribe(waves, batch_size=2, return_hypotheses=True)
    assert len(calls) == n_calls and m.decoding.decoding.fusion_models is None
    assert [(h.y_sequence.tolist(), h.timestamp, h.score) for h in after] == [(h.y_sequence.tolist(), h.timestamp, h.score) for h in before]
