"""Cache-aware streaming inference of the ConformerEncoder: the reference's `setup_streaming_params` / `cache_aware_stream_step`
(modules/conformer_encoder.py) and the `update_cache` paths of its attention and causal depthwise conv, sequenced over the HIP
kernels of csrc/streaming.hip plus the offline path's GEMM / LayerNorm / GLU / norm kernels.

Inference only: no autograd node, no arena, no recorded launch sequences, no packed rows -- one chunk of B streams on the padded
[B, Tq] grid.  Per layer l the caches hold
  cache_last_channel[l] [B, C, d]   the last C frames of the self-attention input (after norm_self_att), C = left context
  cache_last_time[l]    [B, d, K-1] the last K-1 frames of the depthwise conv's input (GLU output, padded frames zeroed)
and a chunk of Tq frames attends to Tk = C + Tq keys: query i sits at key position C + i.

Implemented: att_context_style 'chunked_limited' with a limited left context, causal depthwise conv (conv_context_size 'causal'),
causal down-sampling ('striding' x4 / 'dw_striding' x4, x8).  Everything else raises NotImplementedError naming the option."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List

import torch

from .. import ops
from .conformer_encoder import _Step


@dataclass
class CacheAwareStreamingConfig:
    """the reference's CacheAwareStreamingConfig (same field names and meaning)"""
    chunk_size: List[int] = field(default_factory=lambda: [0, 0])     # mel frames of the first / of every later chunk
    shift_size: List[int] = field(default_factory=lambda: [0, 0])     # mel frames the buffer advances per chunk
    cache_drop_size: int = 0                                           # frames dropped from the end of each output (regular style)
    last_channel_cache_size: int = 0                                   # C: frames in cache_last_channel
    valid_out_len: int = 0                                             # encoder frames a chunk produces
    pre_encode_cache_size: List[int] = field(default_factory=lambda: [0, 0])  # mel frames of the previous input re-fed in front
    drop_extra_pre_encoded: int = 0                                    # sub-sampled frames dropped from the front of a chunk
    last_channel_num: int = 0                                          # layers with a channel cache
    last_time_num: int = 0                                             # layers with a time cache


def check_streamable(enc, att_context_size):
    """NotImplementedError naming the option when the encoder / context cannot be streamed with caches here"""
    if getattr(enc, "self_attention_model", "rel_pos") != "rel_pos":
        raise NotImplementedError(f"cache-aware streaming: self_attention_model={enc.self_attention_model} (implemented: rel_pos)")
    if enc.att_context_style != "chunked_limited":
        raise NotImplementedError(f"cache-aware streaming: att_context_style={enc.att_context_style} (needs cache_drop_size and "
                                  "right-context conv caches; implemented: chunked_limited)")
    if enc.conv_context_size is None or enc.conv_context_size[1] != 0:
        raise NotImplementedError(f"cache-aware streaming: conv_context_size={enc.conv_context_size} (implemented: causal)")
    if not enc.pre_encode.is_causal:
        raise NotImplementedError("cache-aware streaming: causal_downsampling=False (implemented: causal_downsampling=True)")
    left, right = int(att_context_size[0]), int(att_context_size[1])
    if left < 0:
        raise NotImplementedError(f"cache-aware streaming: att_context_size={[left, right]} with an unlimited left context")
    if right < 0:
        raise NotImplementedError(f"cache-aware streaming: att_context_size={[left, right]} with an unlimited right context")


def streaming_config(enc, att_context_size) -> CacheAwareStreamingConfig:
    """setup_streaming_params for chunked_limited attention and causal sub-sampling"""
    check_streamable(enc, att_context_size)
    left, lookahead = int(att_context_size[0]), int(att_context_size[1])
    f = int(enc.subsampling_factor)
    sampling_frames = [1, f]   # ConvSubsampling.get_sampling_frames
    cfg = CacheAwareStreamingConfig()
    cfg.cache_drop_size = 0
    cfg.last_channel_cache_size = left
    cfg.chunk_size = [sampling_frames[0] + f * lookahead, sampling_frames[1] + f * lookahead]
    cfg.shift_size = list(cfg.chunk_size)
    cfg.pre_encode_cache_size = [0, f + 1]   # ConvSubsampling.get_streaming_cache_size (causal)
    cfg.drop_extra_pre_encoded = 1 + (cfg.pre_encode_cache_size[1] - 1) // f
    cfg.valid_out_len = lookahead + 1
    cfg.last_channel_num = cfg.last_time_num = enc.n_layers
    return cfg


def _pos_proj(enc, Tk, W, cdt, dev):
    """linear_pos of the Tk table for every layer ([n_layers, 2Tk-1, dA]): independent of the input, computed once per key"""
    key = (Tk, cdt, str(dev), enc._weights_version, enc._flatp.generation, enc._geometry(cdt))
    cache = enc.__dict__.setdefault("_stream_pos", {})
    p = cache.get(key)
    if p is None:
        if len(cache) >= 8:
            cache.clear()
        p = enc._pos_proj_fwd(enc.pos_enc.table(Tk, dev, cdt), W, cdt, dev)
        cache[key] = p
    return p


def stream_step(enc, mel, length, cache_last_channel, cache_last_time, cache_last_channel_len, drop_extra):
    """one chunk: -> (outputs [B, D, Tq], encoded_lengths, cache_last_channel_next, cache_last_time_next, cache_last_channel_next_len).
    The input caches are read, never written; the next caches are new tensors."""
    if enc.training:
        raise RuntimeError("cache-aware streaming is inference only: call encoder.eval() first")
    cfg = enc.streaming_cfg
    left, right = enc._stream_ctx
    dev = mel.device
    cdt = enc._cdt()
    if cdt == torch.bfloat16 and enc.d_model % 8:
        raise NotImplementedError(f"bf16 compute needs d_model divisible by 8 (got d_model={enc.d_model})")
    d, H, K, nl = enc.d_model, enc.n_heads, enc.conv_kernel_size, enc.n_layers
    C = cfg.last_channel_cache_size
    B = mel.shape[0]
    if tuple(cache_last_channel.shape) != (nl, B, C, d):
        raise ValueError(f"cache_last_channel: expected shape {(nl, B, C, d)}, got {tuple(cache_last_channel.shape)}")
    if tuple(cache_last_time.shape) != (nl, B, d, K - 1):
        raise ValueError(f"cache_last_time: expected shape {(nl, B, d, K - 1)}, got {tuple(cache_last_time.shape)}")
    saved_arena = enc._arena
    enc._arena = None   # (torch's allocator: the step arenas belong to the training sequencer)
    try:
        W, Wf = enc._plan(cdt, dev)
        mel = mel.to(torch.float32).contiguous()
        _, F_, T = mel.shape
        sp = enc.pre_encode._pad
        T1, F1 = ops.half_len(T, sp), ops.half_len(F_, sp)
        lens = enc._lens(length, enc.pre_encode._sampling_num)
        T2, F2 = T, F_
        for _ in range(enc.pre_encode._sampling_num):
            T2, F2 = ops.half_len(T2, sp), ops.half_len(F2, sp)
        S = _Step(B, F_, T, T1, F1, T2, F2, B * T2, cdt)   # (eval, no dropout: the record's defaults)
        # ---- sub-sampling of [pre-encode cache | chunk], then the frames whose receptive field reaches into the padding go
        x = enc._sub_fwd_dw(S, mel, lens, W, cdt, False) if enc.subsampling == "dw_striding" else \
            enc._sub_fwd_striding(S, mel, lens, W, cdt, False)
        drop = max(0, min(int(drop_extra), T2 - 1))
        Tq = T2 - drop
        if drop:
            x = x.view(B, T2, d)[:, drop:].contiguous().view(B * Tq, d)
        chunk_len = (lens[-1] - drop).clamp_(min=0, max=Tq).contiguous()
        cache_len = cache_last_channel_len.to(device=dev, dtype=torch.int64).clamp(min=0, max=C).contiguous()
        M, Tk = B * Tq, C + Tq
        _, dkp, dA = enc._geometry(cdt)
        p_all = _pos_proj(enc, Tk, W, cdt, dev)
        scale = 1.0 / math.sqrt(enc.d_k)
        ch_next = torch.empty(nl, B, C, d, dtype=torch.float32, device=dev)
        t_next = torch.empty(nl, B, d, K - 1, dtype=torch.float32, device=dev)
        ch_in = cache_last_channel.to(torch.float32).contiguous()
        t_in = cache_last_time.to(torch.float32).contiguous()
        no_drop = lambda p, site: ops.NO_DROP   # noqa: E731
        for i, L in enumerate(enc.layers):
            # ff1 / ff2 are never read: the names only fix WHEN the blocks' activations are released (at the top of the next layer,
            # as before) -- this path runs on torch's caching allocator, where an earlier release changes which blocks come next
            ff1 = ff2 = None
            r1, ff1 = enc._ffn_fwd(f"L{i}.ff1", L.feed_forward1, x, L.norm_feed_forward1, S, W, no_drop, 0, M)
            # ---- self-attention against [channel cache | chunk]
            a = L.self_attn
            y2 = enc._ln_fwd(L.norm_self_att, r1, M, d, cdt, dev)[0]
            wq, ldw = W[f"L{i}.att.wqkv"], W.pitch(f"L{i}.att.wqkv")
            bqkv = Wf[f"L{i}.att.bqkv"].view(-1)
            q = torch.empty(M, dA, dtype=cdt, device=dev)
            ops.gemm(y2, wq, q, M, dA, d, d, ldw, dA, bias=bqkv[:dA])
            kv_in = torch.empty(B * Tk, d, dtype=cdt, device=dev)
            ops.stream_cache_assemble(ch_in[i], y2, kv_in, ch_next[i], B, C, Tq, d)
            kv = torch.empty(B * Tk, 2 * dA, dtype=cdt, device=dev)
            ops.gemm(kv_in, wq, kv, B * Tk, 2 * dA, d, d, ldw, 2 * dA, bias=bqkv[dA:], b_off=dA * ldw)
            bu, bv = (a.pos_bias_u, a.pos_bias_v) if dkp == enc.d_k else (Wf[f"L{i}.att.bu"], Wf[f"L{i}.att.bv"])
            ctx = torch.empty(M, dA, dtype=cdt, device=dev)
            ops.stream_attn(q, dA, kv, 2 * dA, dA, p_all[i], dA, bu, bv, cache_len, chunk_len, ctx, dA, B, H, Tq, Tk, dkp, scale,
                            chunk=right + 1, left_chunks=left // (right + 1))
            r2 = torch.empty(M, d, dtype=torch.float32, device=dev)
            ops.gemm(ctx, W[f"L{i}.att.wo"], r2, M, d, dA, dA, W.pitch(f"L{i}.att.wo"), d, bias=a.linear_out.bias,
                     epi=ops.EPI_RESID, aux_in=r1)
            # ---- convolution module with the time cache
            c = L.conv
            y3 = enc._ln_fwd(L.norm_conv, r2, M, d, cdt, dev)[0]
            pw1 = torch.empty(M, 2 * d, dtype=cdt, device=dev)
            ops.gemm(y3, W[f"L{i}.conv.pw1"], pw1, M, 2 * d, d, d, W.pitch(f"L{i}.conv.pw1"), 2 * d, bias=c.pointwise_conv1.bias)
            g = torch.empty(M, d, dtype=cdt, device=dev)
            ops.glu_fwd(pw1, g, chunk_len, Tq, M, d)
            cc = torch.empty(M, d, dtype=cdt, device=dev)
            ops.stream_dwconv(g, t_in[i], c.depthwise_conv.weight, c.depthwise_conv.bias, cc, t_next[i], B, Tq, d, K)
            bn = c.batch_norm
            z = torch.empty(M, d, dtype=cdt, device=dev)
            if enc.conv_norm_type == "layer_norm":
                yln = enc._ln_fwd(bn, cc, M, d, cdt, dev)[0]
                ops.swish_mask_fwd(yln, z, None, Tq, M, d)
            else:
                bmean = torch.empty(d, dtype=torch.float32, device=dev)
                brstd = torch.empty(d, dtype=torch.float32, device=dev)
                ops.bn_eval_stats(bn.running_mean, bn.running_var, bmean, brstd, bn.eps, d)
                ops.bn_swish_fwd(cc, bmean, brstd, bn.weight, bn.bias, z, M, d)
            r3 = torch.empty(M, d, dtype=torch.float32, device=dev)
            ops.gemm(z, W[f"L{i}.conv.pw2"], r3, M, d, d, d, W.pitch(f"L{i}.conv.pw2"), d, bias=c.pointwise_conv2.bias,
                     epi=ops.EPI_RESID, aux_in=r2)
            r4, ff2 = enc._ffn_fwd(f"L{i}.ff2", L.feed_forward2, r3, L.norm_feed_forward2, S, W, no_drop, 5, M)
            x = enc._ln_fwd(L.norm_out, r4, M, d, torch.float32, dev)[0]
        if enc.out_proj is not None:
            out = enc._out_proj_fwd(x, M, dev).view(B, Tq, enc._feat_out).transpose(1, 2)
        else:
            out = x.view(B, Tq, d).transpose(1, 2)
        len_next = torch.clamp(cache_len + Tq, max=C)
        return out, chunk_len, ch_next, t_next, len_next
    finally:
        enc._arena = saved_arena
