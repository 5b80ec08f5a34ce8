"""Cache-aware streaming step of the FastConformer cache-aware recipe's encoder (17 layers, d_model 512, 8 heads, K 9, dw_striding x8
with 256 channels, LayerNorm conv module, [70, 13]: 112 mel frames = 1.12 s of audio per chunk), bf16, on one GPU.  Per batch size:
  * step time from device events after warm-up (a chunk behind a full pre-encode cache, caches filled),
  * kernel launches per step (torch profiler),
  * real-time factor = step time / 1.12 s,
  * the time to stream 20 s of audio chunk by chunk against one offline eval forward of the same audio.

    python tools/stream_bench.py [--batch 1 16 64] [--steps 50] [--warmup 10] [--layers 17] [--json OUT]
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


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def one_setting(enc, B, steps, warmup):
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
    return dict(batch=B, ms_per_step=round(ms, 3), launches_per_step=launches, rtf=round(ms / 1120.0, 5),
                stream_20s_ms=round(ms_stream, 2), offline_20s_ms=round(ms_off, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--layers", type=int, default=17)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    enc = build(args.layers)
    rows = []
    for B in args.batch:
        r = one_setting(enc, B, args.steps, args.warmup)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
