"""Chunking of a batch of processed features for cache-aware streaming: a minimal `CacheAwareStreamingAudioBuffer` (the reference's
name, parts/utils/streaming_utils.py).  Pure host-side indexing over a [B, F, T] tensor; the chunks stay on its device."""
from __future__ import annotations

import math

import torch


class CacheAwareStreamingAudioBuffer:
    """Built from a model (or its encoder) and a batch of processed mel features [B, F, T] with lengths [B].  Iterating yields
    (chunk [B, F, pre-encode cache + chunk frames], chunk_lengths i64 [B]):
      * the first chunk is chunk_size[0] frames behind pre_encode_cache_size[0] (zero) cache frames;
      * every later chunk is shift_size[1] frames behind the last pre_encode_cache_size[1] frames of the previous input;
      * the last chunk is cut at the end of the batch; chunk_lengths = clamp(length - first frame of the chunk, 0, chunk width).
    `drop_extra_pre_encoded` is the value to hand the stream step with the chunk just yielded: 0 for the first one,
    streaming_cfg.drop_extra_pre_encoded for a chunk behind a full pre-encode cache.  Where fewer than pre_encode_cache_size[1]
    frames precede a chunk (a first chunk shorter than the cache: lookahead 0), the cache is cut at frame 0 instead of being
    zero-padded -- zero frames in front of the stream are not the causal convolutions' padding once they have passed a conv and
    its bias -- and the chunk then re-computes a prefix of the stream, so the drop is the number of frames already emitted."""

    def __init__(self, model, processed_signal, processed_signal_length=None):
        enc = getattr(model, "encoder", model)
        if getattr(enc, "streaming_cfg", None) is None:
            enc.setup_streaming_params()
        self.streaming_cfg = enc.streaming_cfg
        if processed_signal.dim() != 3:
            raise ValueError(f"processed_signal: expected [B, F, T], got {tuple(processed_signal.shape)}")
        self.buffer = processed_signal
        B, _, T = processed_signal.shape
        if processed_signal_length is None:
            processed_signal_length = torch.full((B,), T, dtype=torch.int64)
        self.streams_length = torch.as_tensor(processed_signal_length).to(device=processed_signal.device, dtype=torch.int64)
        self.buffer_idx = 0
        self.step = 0
        self.drop_extra_pre_encoded = 0
        self._sampling_num = int(round(math.log2(int(enc.subsampling_factor))))

    def is_buffer_empty(self):
        return self.buffer_idx >= self.buffer.size(-1)

    def __iter__(self):
        cfg = self.streaming_cfg
        while not self.is_buffer_empty():
            first = self.buffer_idx == 0
            chunk_size = cfg.chunk_size[0] if first else cfg.chunk_size[1]
            shift_size = cfg.shift_size[0] if first else cfg.shift_size[1]
            n_cache = cfg.pre_encode_cache_size[0] if first else cfg.pre_encode_cache_size[1]
            if first:
                drop = 0
            elif n_cache <= self.buffer_idx:
                drop = cfg.drop_extra_pre_encoded
            else:   # a prefix of the stream: drop the frames its first buffer_idx mel frames have produced already
                n_cache, drop = self.buffer_idx, self.buffer_idx
                for _ in range(self._sampling_num):
                    drop = drop // 2 + 1
            start = self.buffer_idx - n_cache
            end = min(self.buffer_idx + chunk_size, self.buffer.size(-1))
            if start < 0:   # (a first chunk with pre-encode cache frames: zeros)
                body = self.buffer[:, :, :end]
                chunk = torch.cat((body.new_zeros(body.shape[0], body.shape[1], -start), body), dim=-1)
            else:
                chunk = self.buffer[:, :, start:end]
            self.drop_extra_pre_encoded = drop
            lengths = torch.clamp(self.streams_length - start, min=0, max=chunk.size(-1))
            self.buffer_idx += shift_size
            self.step += 1
            yield chunk.contiguous(), lengths

    def __len__(self):
        cfg, T = self.streaming_cfg, self.buffer.size(-1)
        if T <= cfg.shift_size[0]:
            return 1
        return 1 + -(-(T - cfg.shift_size[0]) // cfg.shift_size[1])
