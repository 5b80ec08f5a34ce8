"""Cache-aware streaming step of the FastConformer cache-aware recipe's encoder (17 layers, d_model 512, 8 heads, K 9, dw_striding x8
with 256 channels, LayerNorm conv module, [70, 13]: 112 mel frames = 1.12 s of audio per chunk), bf16, on one GPU.  Per batch size:
  * step time from device events after warm-up (a chunk behind a full pre-encode cache, caches filled),
  * kernel launches per step (torch profiler),
  * real-time factor = step time / 1.12 s,
  * the time to stream 20 s of audio chunk by chunk against one offline eval forward of the same audio.

`--decoder {none,ctc,rnnt,tdt}` adds the head's step behind the encoder step and reports it separately (`head_ms_per_step`,
`head_launches`): ctc = ConvASRDecoder + per-frame arg-max; rnnt / tdt = the encoder projection GEMM + the resumable greedy search
(ops.rnnt_greedy_decode_stream / ops.tdt_greedy_decode_stream) from a carried decoder state, at the recipe's transducer
geometry (prediction hidden 640, joint hidden 640, vocabulary 1024, max_symbols 10), bf16 weight images.  For the transducer
heads the same 14 frames are also decoded as 14 one-frame chunks (`head_ms_14x1`): everything paid per chunk -- the projection
GEMM, the other launches and the prediction step the kernel reruns at entry -- is in that figure 14 times instead of once, so the
difference bounds the cost of the rerun from above; it does not isolate it.
`--decoder ctc_beam [--beam-size 4 16 64] [--classes 129 1025] [--lm ORDER]`: the CTC head with the resumable prefix beam search
behind it (ConvASRDecoder + mi355x_ctc_beam_decode_stream, with --lm mi355x_ctc_beam_decode_lm_stream and the trigram of the tests'
generator at alpha 0.5), stepped from the state a stream has after eight chunks, with the n-best chased out on every step and, as
`head_ms_no_emit`, with the state advanced only.  One row per (classes, beam size) under `heads`: median, min and max of 7 rounds.

`--decoder {rnnt,tdt} --head-only FRAMES [FRAMES ...] [--lm ORDER] [--boost P]`: no encoder; the transducer head alone on random
encoder output of FRAMES frames per stream (14 = the streaming step, 250 = 20 s offline), the plain search against the search with
shallow fusion (ops.transducer_greedy_decode_fused: --lm, the n-gram model of the tests' generator at alpha 0.5; --boost, a tree
of P three-label phrases taken from the plain search's own output on this input, at alpha 2.0), resumed from the state after one
chunk.  The two are timed in alternating rounds of one process: median, min and max of 7 rounds each, and the labels emitted.
What is timed is the head's step (`decode_ids_stream`): the encoder-projection GEMM with its cast, the same on both sides, and
the search.  The difference of the two times is the fused kernel's; their ratio understates its relative cost by that share.
The heads' weights are the modules' initialisation times 4 (the tests' scale), so that the joint emits labels and the models are
consulted: a flat joint, as `--decoder rnnt` without --head-only builds it, emits blanks only.

`--pred-layers N [N ...]` (default 1; 1..4): the LSTM layers of the transducer heads' prediction network.  With --head-only and
neither --lm nor --boost the head is timed once per layer count on the same input, the counts alternating in the rounds of one
process: per count the median, min and max of 7 rounds, the labels emitted, and the time relative to the first count.  The heads
share the seed, not the hypotheses: every count is another network, so the labels differ and are reported.  Everywhere else the
first count is the one that is built.

    python tools/stream_bench.py [--batch 1 16 64] [--steps 50] [--warmup 10] [--layers 17] [--decoder none] [--json OUT]
                                 [--beam-size 4 16 64] [--classes 129 1025] [--lm ORDER] [--boost P] [--head-only FRAMES ...]
                                 [--pred-layers N ...]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

dev = "cuda"


def build(n_layers):
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    torch.manual_seed(0)
    enc = ConformerEncoder(feat_in=80, n_layers=n_layers, d_model=512, n_heads=8, conv_kernel_size=9, subsampling="dw_striding",
                           subsampling_factor=8, subsampling_conv_channels=256, causal_downsampling=True,
                           att_context_size=[[70, 13], [70, 6], [70, 1], [70, 0]], att_context_style="chunked_limited",
                           conv_context_size="causal", conv_norm_type="layer_norm", dropout=0.0, dropout_pre_encoder=0.0,
                           dropout_emb=0.0, dropout_att=0.0, compute_dtype=torch.bfloat16)
    enc = enc.to(dev).eval()
    enc.setup_streaming_params(att_context_size=[70, 13])
    return enc


def build_head(kind, d_model=512, fusion_models=None, scale=1.0, pred_layers=1):
    """-> step(encoded [B, D, T], encoded_len) for the head `kind`, weights random (the step's cost does not depend on them much:
    the transducer search emits what a random joint emits, bounded by max_symbols = 10 per frame)"""
    from nemo_amd.modules import ConvASRDecoder, GreedyBatchedRNNTInfer, GreedyBatchedTDTInfer, RNNTDecoder, RNNTJoint
    torch.manual_seed(1)
    V = 1024
    if kind == "ctc":
        dec = ConvASRDecoder(feat_in=d_model, num_classes=V, compute_dtype=torch.bfloat16).to(dev).eval()
        return lambda enc, n, state=None: (dec(encoder_output=enc).argmax(-1), None)
    durations = [0, 1, 2, 3, 4]
    pred = RNNTDecoder(prednet={"pred_hidden": 640, "pred_rnn_layers": pred_layers, "dropout": 0.0}, vocab_size=V,
                       compute_dtype=torch.bfloat16)
    joint = RNNTJoint(jointnet={"encoder_hidden": d_model, "pred_hidden": 640, "joint_hidden": 640, "activation": "relu", "dropout": 0.0},
                      num_classes=V, num_extra_outputs=len(durations) if kind == "tdt" else 0, compute_dtype=torch.bfloat16)
    with torch.no_grad():
        for p in list(pred.parameters()) + list(joint.parameters()):   # (scale 1: a nearly flat joint, which the blank bias decides)
            p.mul_(scale)
        joint.joint_net[-1].bias[V] += 2.0   # (a blank now and then, as a trained model has)
    pred, joint = pred.to(dev).eval(), joint.to(dev).eval()
    infer = (GreedyBatchedTDTInfer(pred, joint, V, durations, max_symbols_per_step=10, fusion_models=fusion_models) if kind == "tdt"
             else GreedyBatchedRNNTInfer(pred, joint, V, max_symbols_per_step=10, fusion_models=fusion_models))

    def step(enc, n, state=None, lengths=False):
        tokens, times, out_len, nxt, *_ = infer.decode_ids_stream(enc, n, state)
        return ((tokens, out_len) if lengths else tokens), nxt
    return step


def layers_head_setting(kind, layer_counts, B, frames, steps, warmup, n_rounds=7, d_model=512):
    """the transducer head alone on `frames` frames per stream, once per count of prediction-network layers, alternating rounds"""
    import statistics
    g = torch.Generator(device=dev).manual_seed(2)
    enc_out = torch.randn(B, d_model, frames, device=dev, generator=g)
    enc_len = torch.full((B,), frames, dtype=torch.int64, device=dev)
    row = dict(decoder=kind, batch=B, frames=frames, layers=[])
    with torch.no_grad():
        fns, labels = {}, {}
        for L in layer_counts:
            head = build_head(kind, d_model, scale=4.0, pred_layers=L)
            (_, out_len), state = head(enc_out, enc_len, lengths=True)
            labels[L] = int(out_len.sum())
            fns[L] = lambda head=head, state=state: head(enc_out, enc_len, state)
        for fn in fns.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        ms = {L: [] for L in fns}
        for _ in range(n_rounds):
            for L, fn in fns.items():
                ms[L].append(timed(fn, steps))
    first = statistics.median(ms[layer_counts[0]])
    for L, v in ms.items():
        med = statistics.median(v)
        row["layers"].append(dict(pred_layers=L, labels=labels[L], ms=round(med, 3), ms_range=[round(min(v), 3), round(max(v), 3)],
                                  ratio=round(med / first, 3)))
    return row


def fused_head_setting(kind, lm_order, n_phrases, B, frames, steps, warmup, n_rounds=7, d_model=512, pred_layers=1):
    """the transducer head alone on `frames` frames per stream: the plain search against the fused one, alternating rounds"""
    import statistics
    V = 1024
    g = torch.Generator(device=dev).manual_seed(2)
    enc_out = torch.randn(B, d_model, frames, device=dev, generator=g)
    enc_len = torch.full((B,), frames, dtype=torch.int64, device=dev)
    # (the tests' scale: a joint that emits labels, so that the models are consulted)
    plain = build_head(kind, d_model, scale=4.0, pred_layers=pred_layers)
    with torch.no_grad():
        (tokens, out_len), p_state = plain(enc_out, enc_len, lengths=True)
    models = []
    if lm_order:
        from ctc_beam_bench import make_ngram_lm
        models.append((make_ngram_lm(V, lm_order), 0.5))
    if n_phrases:   # runs of three labels the plain search emits on this input: phrases that are walked, completed and broken off
        from nemo_amd.modules import BoostingTree
        tokens, out_len = tokens.cpu(), out_len.cpu()
        runs = [tuple(tokens[b, i:i + 3].tolist()) for b in range(B) for i in range(0, int(out_len[b]) - 2, 3)]
        runs = list(dict.fromkeys(runs))[:n_phrases]
        models.append((BoostingTree.from_phrases(runs, V), 2.0))
    fused = build_head(kind, d_model, fusion_models=models, scale=4.0, pred_layers=pred_layers)   # (the same seed: the same weights)
    row = dict(decoder=kind, batch=B, frames=frames, lm_order=lm_order, phrases=len(models[-1][0].phrases) if n_phrases else 0,
               pred_layers=pred_layers)
    with torch.no_grad():
        (_, f_len), f_state = fused(enc_out, enc_len, lengths=True)
        row["labels_plain"], row["labels_fused"] = int(out_len.sum()), int(f_len.sum())
        fns = dict(plain=lambda: plain(enc_out, enc_len, p_state), fused=lambda: fused(enc_out, enc_len, f_state))
        for fn in fns.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        ms = dict(plain=[], fused=[])
        for _ in range(n_rounds):
            for name, fn in fns.items():
                ms[name].append(timed(fn, steps))
    for name, v in ms.items():
        row[name + "_ms"] = round(statistics.median(v), 3)
        row[name + "_ms_range"] = [round(min(v), 3), round(max(v), 3)]
    return row


def build_beam_head(C, W, lm_order, d_model=512):
    """-> step(encoded, encoded_len, state, emit) for the CTC head over C classes with the resumable beam search of width W"""
    from nemo_amd.modules import BeamBatchedCTCDecoder, ConvASRDecoder
    torch.manual_seed(1)
    dec = ConvASRDecoder(feat_in=d_model, num_classes=C - 1, compute_dtype=torch.bfloat16).to(dev).eval()
    with torch.no_grad():
        dec.decoder_layers[0].weight.mul_(8.0)   # (random weights give nearly flat rows: peaked ones, so that the threshold prunes)
    lm = None
    if lm_order:
        from ctc_beam_bench import make_ngram_lm
        lm = make_ngram_lm(C - 1, lm_order)
    search = BeamBatchedCTCDecoder(blank_id=C - 1, beam_size=W, ngram_lm=lm, ngram_lm_alpha=0.5 if lm else 0.0)
    return lambda enc, n, state=None, emit=True: search.decode_stream(dec(encoder_output=enc), n, state, emit=emit)


def beam_head_setting(head, enc_out, enc_len, steps, warmup, n_rounds=7):
    import statistics
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad():
        state = None
        for _ in range(8):   # a stream in mid-flight: the tree holds eight chunks
            _, state = head(enc_out, enc_len, state)
        row = {}
        for key, emit in (("head_ms_per_step", True), ("head_ms_no_emit", False)):
            fn = lambda: head(enc_out, enc_len, state, emit)   # noqa: E731  (out of place: every call is the same step)
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            ms = [timed(fn, steps) for _ in range(n_rounds)]
            row[key] = round(statistics.median(ms), 3)
            row[key + "_range"] = [round(min(ms), 3), round(max(ms), 3)]
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            head(enc_out, enc_len, state)
            torch.cuda.synchronize()
        row["head_launches"] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        row["chunk_frames"] = int(enc_out.shape[2])
    return row


def head_setting(head, kind, B, enc_out, enc_len, steps, warmup):
    """the head's step on one encoder chunk output (device time, launches), and for transducers the same frames as one-frame chunks"""
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad():
        _, state = head(enc_out, enc_len)
        fn = lambda: head(enc_out, enc_len, state)   # noqa: E731
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, steps)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        row = dict(head_ms_per_step=round(ms, 3), head_launches=launches)
        if kind in ("rnnt", "tdt"):
            T = enc_out.shape[2]
            frames = [enc_out[:, :, t:t + 1].contiguous() for t in range(T)]
            one = torch.ones_like(enc_len)

            def by_frame():
                st = state
                for f in frames:
                    _, st = head(f, one, st)
            by_frame()
            torch.cuda.synchronize()
            row["head_ms_14x1"] = round(timed(by_frame, max(2, steps // 5)), 3)
            row["chunk_frames"] = T
    return row


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def one_setting(enc, B, steps, warmup, head=None, kind="none"):
    from torch.profiler import ProfilerActivity, profile
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    cfg = enc.streaming_cfg
    g = torch.Generator(device=dev).manual_seed(1)
    width = cfg.pre_encode_cache_size[1] + cfg.shift_size[1]
    chunk = torch.randn(B, 80, width, device=dev, generator=g)
    clen = torch.full((B,), width, dtype=torch.int64, device=dev)
    ch, tm, ln = enc.get_initial_cache_state(batch_size=B)
    ch.normal_(generator=g)
    tm.normal_(generator=g)
    ln.fill_(cfg.last_channel_cache_size)

    def step():
        return enc.cache_aware_stream_step(processed_signal=chunk, processed_signal_length=clen, cache_last_channel=ch,
                                           cache_last_time=tm, cache_last_channel_len=ln)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = timed(step, steps)
    head_row = {}
    if kind == "ctc_beam":   # `head`: [(settings, step)], one per (classes, beam size)
        res = step()
        head_row = dict(heads=[dict(cfg, **beam_head_setting(h, res[0].detach(), res[1].detach(), steps, warmup)) for cfg, h in head])
    elif head is not None:
        res = step()
        head_row = head_setting(head, kind, B, res[0].detach(), res[1].detach(), steps, warmup)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    # 20 s of audio: streamed chunk by chunk vs one offline forward
    T = 2000
    mel = torch.randn(B, 80, T, device=dev, generator=g)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)

    def stream_all():
        c, t, n = enc.get_initial_cache_state(batch_size=B)
        buf = CacheAwareStreamingAudioBuffer(enc, mel, lens)
        for x, xl in buf:
            _, _, c, t, n = enc.cache_aware_stream_step(processed_signal=x, processed_signal_length=xl, cache_last_channel=c,
                                                        cache_last_time=t, cache_last_channel_len=n,
                                                        drop_extra_pre_encoded=buf.drop_extra_pre_encoded)

    def offline():
        with torch.no_grad():
            enc(audio_signal=mel, length=lens)
    stream_all(); offline()
    torch.cuda.synchronize()
    ms_stream = timed(stream_all, 2)
    ms_off = timed(offline, 3)
    row = dict(batch=B, ms_per_step=round(ms, 3), launches_per_step=launches, rtf=round(ms / 1120.0, 5),
               stream_20s_ms=round(ms_stream, 2), offline_20s_ms=round(ms_off, 2))
    if kind == "ctc_beam":
        row.update(decoder=kind, **head_row)
    elif head_row:
        row.update(decoder=kind, **head_row)
        row["rtf_with_head"] = round((ms + head_row["head_ms_per_step"]) / 1120.0, 5)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--layers", type=int, default=17)
    ap.add_argument("--decoder", choices=["none", "ctc", "rnnt", "tdt", "ctc_beam"], default="none")
    ap.add_argument("--beam-size", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--classes", type=int, nargs="+", default=[129, 1025])
    ap.add_argument("--lm", type=int, default=0, metavar="ORDER")
    ap.add_argument("--boost", type=int, default=0, metavar="P")
    ap.add_argument("--head-only", type=int, nargs="+", default=None, metavar="FRAMES")
    ap.add_argument("--pred-layers", type=int, nargs="+", default=[1], metavar="N", choices=[1, 2, 3, 4])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.head_only:
        if args.decoder not in ("rnnt", "tdt"):
            ap.error("--head-only times the transducer heads: --decoder rnnt|tdt (with --lm and / or --boost: with and without "
                     "fusion; without them: per --pred-layers count)")
        rows = []
        for B in args.batch:
            for frames in args.head_only:
                if args.lm or args.boost:
                    rows.append(fused_head_setting(args.decoder, args.lm, args.boost, B, frames, args.steps, args.warmup,
                                                   pred_layers=args.pred_layers[0]))
                else:
                    rows.append(layers_head_setting(args.decoder, args.pred_layers, B, frames, args.steps, args.warmup))
                print(json.dumps(rows[-1]), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(rows, f, indent=1)
        return
    enc = build(args.layers)
    if args.decoder == "ctc_beam":
        head = [(dict(classes=C, beam_size=W, lm_order=args.lm), build_beam_head(C, W, args.lm)) for C in args.classes
                for W in args.beam_size]
    else:
        head = build_head(args.decoder, pred_layers=args.pred_layers[0]) if args.decoder != "none" else None
    rows = []
    for B in args.batch:
        r = one_setting(enc, B, args.steps, args.warmup, head, args.decoder)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
