"""-m gpu: EncDecHybridRNNTCTCModel -- both heads in one training step, and cache-aware streaming with either head."""
import contextlib

import pytest
import torch

from oracle import conformer_ref as R
from oracle import transducer_ref as TR

import stream_decode_oracle as S

pytestmark = pytest.mark.gpu
dev = "cuda"
LABELS = [chr(ord("a") + i) for i in range(26)] + [" ", "'"]


def _cfg(w, cdt=torch.float32, fused=False, tdt=False, **enc):
    from nemo_amd.models import fastconformer_hybrid_config
    over = dict(d_model=64, n_heads=4, n_layers=2, subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0,
                compute_dtype=cdt)
    over.update(enc)
    cfg = fastconformer_hybrid_config("small", vocab_size=len(LABELS), ctc_loss_weight=w, durations=[0, 1, 2, 3, 4] if tdt else None,
                                      **over)
    cfg["labels"] = LABELS
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    cfg["joint"]["fuse_loss_wer"] = fused
    cfg["joint"]["fused_batch_size"] = 2
    return cfg


def _batch():
    audio, _, tok, _ = R.synthetic_batch(4, 1.5, vocab=len(LABELS), seed=3)
    alen = torch.tensor([24000, 20000, 24000, 12000]); tl = torch.tensor([4, 3, 4, 2])
    return [audio.to(dev), alen.to(dev), tok[:, :4].contiguous().to(dev), tl.to(dev)]


def _step_grads(m, batch):
    """zero the flat gradients, one training_step + backward as fit_step runs them -> (step output, flat gradients per module)"""
    for fp in m.flats():
        fp.zero_grad()
    scope = getattr(m.encoder, "step_scope", None)
    with (scope() if scope is not None else contextlib.nullcontext()):
        out = m.training_step(batch, 0)
        out["loss"].backward()
    m._after_backward()
    if hasattr(m.encoder, "_wgrad_join"):
        m.encoder._wgrad_join()
    torch.cuda.synchronize()
    return out, [fp.grad.detach().clone() for fp in m.flats()]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _pair(w, fused=False, tdt=False):
    from nemo_amd.models import EncDecHybridRNNTCTCModel, EncDecRNNTModel
    cfg = _cfg(w, fused=fused, tdt=tdt)
    torch.manual_seed(4)
    hyb = EncDecHybridRNNTCTCModel(cfg)
    pcfg = {k: v for k, v in cfg.items() if k != "aux_ctc"}
    par = EncDecRNNTModel(pcfg)
    par.load_state_dict({k: v for k, v in hyb.state_dict().items() if not k.startswith("ctc_decoder.")})
    for m in (hyb, par):
        m.decoder.compute_dtype = m.joint.compute_dtype = torch.float32
    return hyb.to(dev).train(), par.to(dev).train()


@pytest.mark.parametrize("fused,tdt", [(False, False), (True, False), (False, True)])
def test_hybrid_with_ctc_weight_zero_is_the_transducer_model(fused, tdt):
    """ctc_loss_weight = 0: loss and the gradients of encoder, prediction network and joint equal EncDecRNNTModel's with the same
    weights; the CTC head is not run (its gradient stays zero, no train_ctc_loss is logged).
    Parent and hybrid are each run eight times.  What all sixteen runs reproduce bit for bit (on the MI355X: the loss and the
    joint's flat gradient) must be bit-equal between the two models.  The other gradients are not reproducible run to run (atomic
    accumulation in the backward; relative L2 difference between two parent runs: encoder 0.9e-8 .. 1.9e-8, prediction network
    2.9e-8 .. 4.4e-8, every pair about the same distance apart).  There the hybrid must agree with the parent within the parent's
    own run-to-run difference: the smallest of the 64 hybrid-to-parent distances may not exceed the largest of the 28
    parent-to-parent distances, per module.  An earlier form compared ONE hybrid run with the nearest of the parent runs; distances
    between such noise vectors concentrate around one value, so that form failed by chance (3.29e-8 against 3.27e-8 for the
    prediction network, once in a clean run of the suite).  With 64 samples against 28 of the same distribution the comparison
    no longer hangs on one draw, while a real difference between the models (1e-3 and more) shifts all 64."""
    hyb, par = _pair(0.0, fused=fused, tdt=tdt)
    batch = _batch()
    n_runs = 8
    runs = [_step_grads(par, batch) for _ in range(n_runs)]
    hruns = [_step_grads(hyb, batch) for _ in range(n_runs)]
    pairs = [(i, j) for i in range(n_runs) for j in range(i)]
    for oh, gh in hruns:
        assert "train_ctc_loss" not in oh["log"] and torch.equal(oh["log"]["train_rnnt_loss"], oh["log"]["train_loss"])
        assert not gh[3].any()
    losses_p, losses_h = [r[0]["loss"].item() for r in runs], [r[0]["loss"].item() for r in hruns]
    self_loss = max(abs(a - b) for a in losses_p for b in losses_p)
    print("parent run-to-run difference: loss", self_loss)
    if len(set(losses_p)) == 1 and len(set(losses_h)) == 1:
        assert losses_p[0] == losses_h[0]
    else:
        assert min(abs(a - b) for a in losses_h for b in losses_p) <= self_loss
    for k in range(3):
        self_grad = max(_rel(runs[i][1][k], runs[j][1][k]) for i, j in pairs)
        self_hyb = max(_rel(hruns[i][1][k], hruns[j][1][k]) for i, j in pairs)
        cross = [_rel(h[1][k], r[1][k]) for h in hruns for r in runs]
        print("module", k, "parent-to-parent max", self_grad, "hybrid-to-hybrid max", self_hyb, "hybrid-to-parent min / max",
              min(cross), max(cross))
        if self_grad == 0.0 and self_hyb == 0.0:   # bit-stable over all sixteen runs
            assert torch.equal(hruns[0][1][k], runs[0][1][k]), k
        else:
            assert min(cross) <= self_grad, (k, min(cross), self_grad)


def test_hybrid_step_combines_both_heads():
    """ctc_loss_weight = 0.3, fp32, un-fused joint.  Logged losses = what the existing loss modules give on the same `encoded`;
    train_loss = their weighted sum; the gradient at `encoded` and the ctc_decoder gradients against the float64 combination
    (1 - w) * g_rnnt + w * g_ctc of the heads' separately computed gradients.  Allowance per tensor: 4 x the relative L2 difference
    between the gradient under a loss scaled by the head's weight and the weight times the unscaled gradient (what a scale alone
    costs in rounding; for `encoded` measured on the transducer path with 1 - w, for the ctc_decoder buffer on the CTC path with
    w), covering the second head and the add.  Measured on an MI355X: scale cost 1.5e-7 (encoded) and 1.7e-7 (ctc_decoder), so
    the allowances are 6.0e-7 and 6.7e-7; the differences came out at 1.2e-7 and 1.7e-7."""
    from nemo_amd.models import EncDecRNNTModel
    w = 0.3
    hyb, _ = _pair(w)
    batch = _batch()
    seen = {}
    fwd = hyb.forward

    def forward(**kw):
        enc, enc_len = fwd(**kw)
        enc.retain_grad()
        seen["enc"], seen["len"] = enc, enc_len
        return enc, enc_len
    hyb.forward = forward
    out, grads = _step_grads(hyb, batch)
    hyb.forward = fwd
    enc, enc_len = seen["enc"], seen["len"]
    g_enc, g_ctcp = enc.grad.detach().clone(), grads[3]
    _, _, tr, trl = batch

    def rnnt_head(scale):
        e = enc.detach().clone().requires_grad_(True)
        d, tl, _ = hyb.decoder(targets=tr, target_length=trl)
        loss = EncDecRNNTModel._loss_and_wer(hyb, e, enc_len, d, tl, tr, trl, False)[0]
        (loss * scale if scale != 1.0 else loss).backward()
        torch.cuda.synchronize()
        return loss.detach(), e.grad.detach().clone()

    def ctc_head(scale):
        hyb.ctc_decoder.flat_parameters().zero_grad()
        e = enc.detach().clone().requires_grad_(True)
        loss = hyb.ctc_loss(log_probs=hyb.ctc_decoder(encoder_output=e), targets=tr, input_lengths=enc_len, target_lengths=trl)
        (loss * scale if scale != 1.0 else loss).backward()
        torch.cuda.synchronize()
        return loss.detach(), e.grad.detach().clone(), hyb.ctc_decoder.flat_parameters().grad.detach().clone()
    r_loss, g_r = rnnt_head(1.0)
    _, g_r_scaled = rnnt_head(1.0 - w)
    c_loss, g_c, p_c = ctc_head(1.0)
    _, _, p_c_scaled = ctc_head(w)
    log = out["log"]
    assert torch.equal(log["train_rnnt_loss"], r_loss) and torch.equal(log["train_ctc_loss"], c_loss)
    torch.testing.assert_close(log["train_loss"], (1 - w) * r_loss + w * c_loss)
    cost_enc, cost_ctc = _rel(g_r_scaled, (1 - w) * g_r.double()), _rel(p_c_scaled, w * p_c.double())
    d_enc = _rel(g_enc, (1 - w) * g_r.double() + w * g_c.double())
    d_ctc = _rel(g_ctcp, w * p_c.double())
    print(f"scale cost: encoded {cost_enc:.3e}, ctc_decoder {cost_ctc:.3e}; difference: encoded {d_enc:.3e}, ctc_decoder {d_ctc:.3e}")
    assert d_enc <= 4 * cost_enc and d_ctc <= 4 * cost_ctc


@pytest.mark.parametrize("tdt", [False, True])
def test_hybrid_bf16_fit_step_with_the_fused_joint_trains_all_four_modules(tdt):
    from nemo_amd.models import EncDecHybridRNNTCTCModel
    cfg = _cfg(0.3, cdt=torch.bfloat16, fused=True, tdt=tdt)
    cfg["log_every_n_steps"] = 1
    torch.manual_seed(6)
    m = EncDecHybridRNNTCTCModel(cfg)
    m.decoder.compute_dtype = m.joint.compute_dtype = m.ctc_decoder.compute_dtype = torch.bfloat16
    m = m.to(dev).train()
    m.setup_optimization(dict(name="adamw", lr=1e-3, betas=[0.9, 0.98], weight_decay=0.0))
    before = [fp.flat.detach().clone() for fp in m.flats()]
    out = m.fit_step(_batch())
    torch.cuda.synchronize()
    log = out["log"]
    assert torch.isfinite(out["loss"]) and torch.isfinite(log["train_rnnt_loss"]) and torch.isfinite(log["train_ctc_loss"])
    assert "training_batch_wer" in log and "training_batch_wer_ctc" in log
    assert len(before) == 4
    for b, fp in zip(before, m.flats()):
        assert not torch.equal(b, fp.flat)
    m.eval()
    v = m.validation_pass(_batch())
    assert {"val_loss", "val_wer", "val_wer_ctc", "val_wer_num_ctc", "val_wer_denom_ctc"} <= set(v)


# ------------------------------------------------------------------------------------------------ streaming
def _stream_model(seed):
    """a small cache-aware encoder as in tests/test_streaming_gpu.py::test_ctc_conformer_stream_step_matches_offline_greedy; the
    transducer head sized as tests/test_rnnt_decoding.py sizes its search case (parameters x 4, blank bias raised)"""
    from nemo_amd.models import EncDecHybridRNNTCTCModel
    from test_streaming_gpu import _randomise
    cfg = _cfg(0.3, subsampling="striding", subsampling_factor=4, causal_downsampling=True, att_context_size=[16, 3],
               att_context_style="chunked_limited", conv_kernel_size=9, conv_context_size="causal")
    torch.manual_seed(seed)
    m = EncDecHybridRNNTCTCModel(cfg)
    _randomise(m.encoder, seed + 1)
    with torch.no_grad():
        for p in list(m.decoder.parameters()) + list(m.joint.parameters()):
            p.mul_(4.0)
        m.joint.joint_net[-1].bias[len(LABELS)] += 2.0
    m.decoder.compute_dtype = m.joint.compute_dtype = torch.float32
    return m.to(dev).eval()


def _audio():
    g = torch.Generator().manual_seed(13)
    return (0.1 * torch.randn(3, 48000, generator=g)).to(dev), torch.tensor([48000, 34000, 18000]).to(dev)


def test_hybrid_stream_step_ctc_head_matches_offline_greedy():
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    m = _stream_model(11)
    m.change_decoding_strategy(decoder_type="ctc")
    audio, alen = _audio()
    with torch.no_grad():
        mel, mel_len = m.preprocessor(input_signal=audio, length=alen)
        enc_off, enc_len = m.forward(processed_signal=mel, processed_signal_length=mel_len)
        lp = m.ctc_decoder(encoder_output=enc_off)
    ch, tm, ln = m.encoder.get_initial_cache_state(batch_size=3)
    prev = None
    buf = CacheAwareStreamingAudioBuffer(m, mel, mel_len)
    for chunk, cl in buf:
        preds, texts, ch2, tm2, ln2, best = m.conformer_stream_step(
            processed_signal=chunk, processed_signal_length=cl, cache_last_channel=ch, cache_last_time=tm, cache_last_channel_len=ln,
            previous_pred_out=prev, drop_extra_pre_encoded=buf.drop_extra_pre_encoded, return_transcription=True)
        assert best is None and len(texts) == 3
        for a, b in ((ch, ch2), (tm, tm2), (ln, ln2)):
            assert a.data_ptr() != b.data_ptr()
        ch, tm, ln, prev = ch2, tm2, ln2, preds
    torch.cuda.synchronize()
    top2 = lp.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]).cpu()
    off_pred = lp.argmax(-1).cpu()
    for b in range(3):
        L = int(enc_len[b])
        assert prev[b].numel() == L
        diff = (prev[b] != off_pred[b, :L]) & (margin[b, :L] >= 1e-4)   # the existing test's criterion
        assert not diff.any(), (b, diff.nonzero())


def test_hybrid_stream_step_transducer_head():
    """Streamed hypotheses (three utterances of different length, decoder state carried in the hypotheses) against
      * one launch over the collected streamed encoder outputs: equal where the per-chunk projection GEMM gives the whole-sequence
        values, and in any case within the rules of tests/test_rnnt_decoding.py (rule 2) along the CPU restatement;
      * the offline forward: the streamed hypotheses walked through forced_decode_margins on the OFFLINE encoder output -- every
        differing decision within 2e-4 * scale, at most 2 % differing, no utterance left out.
    Seeds tried for the model: 11 (the first)."""
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    m = _stream_model(11)
    V, ms = len(LABELS), 10
    audio, alen = _audio()
    with torch.no_grad():
        mel, mel_len = m.preprocessor(input_signal=audio, length=alen)
        enc_off, enc_len = m.forward(processed_signal=mel, processed_signal_length=mel_len)
    Pd = {k: v.detach().float().cpu() for k, v in m.decoder.state_dict().items()}
    Pj = {k: v.detach().float().cpu() for k, v in m.joint.state_dict().items()}
    enc_off_c, enc_len_c = enc_off.float().cpu(), enc_len.cpu()
    # the fp32 search on the offline output is not a near-tie lottery (the condition of the 2 % rule)
    gaps = []
    S.decode_chunked(Pd, Pj, enc_off_c, enc_len_c, V, ms, [], gaps=gaps)
    near = sum(1 for gap, scale in gaps if gap < 2e-4 * scale)
    print("offline fp32 search: decisions", len(gaps), "near-ties", near)
    assert len(gaps) > 150 and near < 0.02 * len(gaps)
    # stream, recording the encoder's chunk outputs
    rec = []
    step = m.encoder.cache_aware_stream_step

    def recording(**kw):
        res = step(**kw)
        rec.append((res[0].detach().clone(), res[1].detach().clone()))
        return res
    m.encoder.cache_aware_stream_step = recording
    ch, tm, ln = m.encoder.get_initial_cache_state(batch_size=3)
    hyps = None
    buf = CacheAwareStreamingAudioBuffer(m, mel, mel_len)
    try:
        for chunk, cl in buf:
            before = None if hyps is None else [(h.y_sequence.clone(), list(h.timestamp), h.score) for h in hyps]
            chunk0, caches0 = chunk.clone(), [x.clone() for x in (ch, tm, ln)]
            state0 = None if hyps is None else [[t.clone() for t in h.dec_state.tensors()] for h in hyps]
            preds, new, ch2, tm2, ln2, best = m.conformer_stream_step(
                processed_signal=chunk, processed_signal_length=cl, cache_last_channel=ch, cache_last_time=tm,
                cache_last_channel_len=ln, previous_hypotheses=hyps, drop_extra_pre_encoded=buf.drop_extra_pre_encoded)
            assert torch.equal(chunk, chunk0) and best is new and all(torch.equal(p, h.y_sequence) for p, h in zip(preds, new))
            for a, b, a0 in ((ch, ch2, caches0[0]), (tm, tm2, caches0[1]), (ln, ln2, caches0[2])):
                assert a.data_ptr() != b.data_ptr() and torch.equal(a, a0)   # new cache objects, the old ones as they were
            if hyps is not None:
                for h, n, (y, ts, sc), st0 in zip(hyps, new, before, state0):
                    assert h is not n and torch.equal(h.y_sequence, y) and h.timestamp == ts and h.score == sc
                    assert all(torch.equal(t, t0) for t, t0 in zip(h.dec_state.tensors(), st0))
            ch, tm, ln, hyps = ch2, tm2, ln2, new
    finally:
        m.encoder.cache_aware_stream_step = step
    with pytest.raises(NotImplementedError):
        m.conformer_stream_step(processed_signal=chunk, processed_signal_length=cl, cache_last_channel=ch, cache_last_time=tm,
                                cache_last_channel_len=ln, return_log_probs=True)
    torch.cuda.synchronize()
    assert len(rec) >= 3
    got = [(h.y_sequence.tolist(), h.timestamp) for h in hyps]
    assert all(isinstance(h.text, str) for h in hyps)
    # the collected streamed encoder output, decoded in one launch
    Tm, D = int(enc_len.max()), enc_off.shape[1]
    coll = torch.zeros(3, D, Tm, device=dev)
    fill = [0, 0, 0]
    infer = m.decoding.decoding
    same_proj, spans = True, []
    for e, l in rec:
        fch = infer._project(e)[0]
        for b in range(3):
            n = int(l[b])
            coll[b, :, fill[b]:fill[b] + n] = e[b, :, :n]
            spans.append((b, fill[b], n, fch[b, :n]))
            fill[b] += n
    assert fill == enc_len_c.tolist()   # every stream produced the offline number of frames
    f_whole = infer._project(coll)[0]
    for b, lo, n, fch in spans:
        same_proj &= torch.equal(fch, f_whole[b, lo:lo + n])
    one = m.decoding.rnnt_decoder_predictions_tensor(coll, enc_len)
    if same_proj:
        for h, o in zip(hyps, one):
            assert torch.equal(h.y_sequence, o.y_sequence) and h.timestamp == o.timestamp and h.score == o.score
    # the same chunks decoded again with the projection step handing out slices of the whole-sequence projection: equal to the one
    # launch, unconditionally
    _, args = infer._project(coll)
    project = infer._project
    hyps2, off = infer.fresh_hypotheses(3), [0, 0, 0]
    try:
        for e, l in rec:
            fc = torch.zeros(3, e.shape[2], f_whole.shape[2], dtype=f_whole.dtype, device=dev)
            for b in range(3):
                n = int(l[b])
                fc[b, :n] = f_whole[b, off[b]:off[b] + n]
                off[b] += n
            infer._project = lambda chunk, fc=fc: (fc, args)
            hyps2 = m.decoding.rnnt_decoder_predictions_tensor(e, l, return_hypotheses=True, partial_hypotheses=hyps2)
    finally:
        infer._project = project
    for h, o in zip(hyps2, one):
        assert torch.equal(h.y_sequence, o.y_sequence) and h.timestamp == o.timestamp and h.score == o.score and h.text == o.text
    rep = TR.forced_decode_margins(Pd, Pj, coll.cpu(), enc_len_c, V, ms, got)
    _rule2(rep, "streamed output", sum(len(g[0]) for g in got))
    print("per-chunk projection equals the whole-sequence one:", same_proj)
    # against the offline forward
    rep = TR.forced_decode_margins(Pd, Pj, enc_off_c, enc_len_c, V, ms, got)
    assert len(rep) == 3
    _rule2(rep, "offline output", sum(len(g[0]) for g in got))


def _rule2(rep, what, n_labels):
    decisions = [r for rows in rep for r in rows]
    flips = [r for r in decisions if r[1] != r[2]]
    print(what, "flips / decisions:", len(flips), len(decisions), "largest margin / scale:",
          max([r[3] / r[4] for r in flips], default=0.0))
    assert len(decisions) > 150 and n_labels > 40, (what, len(decisions), n_labels)
    for t, follow, own, margin, scale in flips:
        assert margin <= 2e-4 * scale, (what, t, follow, own, margin, scale)
    assert len(flips) <= 0.02 * len(decisions), (what, len(flips), len(decisions))
