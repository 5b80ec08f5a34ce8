"""TEST INFRASTRUCTURE ONLY -- plain-torch restatement of one cache-aware streaming step of the ConformerEncoder (the reference's
`cache_aware_stream_step` with the `update_cache` paths of RelPositionMultiHeadAttention and CausalConv1D), built on the pieces of
oracle/conformer_ref.py.  The caches are explicit torch.cat operations:

  channel cache  keys / values of a chunk = cat(cache_last_channel[l], LN_self_att(x)) along time (Tk = C + Tq rows); query i sits
                 at key position C + i; the next cache is the last C rows
  time cache     the depthwise conv's input = cat(cache_last_time[l], GLU output) along time, convolved without padding; the next
                 cache is the last K-1 frames

Runs in the dtype of the parameters (float64 in the host tests)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import conformer_ref as R
from oracle import squeezeformer_ref as SQ


def subsample(P, cfg, mel, mel_len, subsampling):
    """causal sub-sampling stack of the encoder -> ([B, T', d], lengths)"""
    if subsampling == "dw_striding":
        return SQ.dw_striding_forward(P, mel, mel_len, cfg=cfg)
    return R.subsampling_forward(P, cfg, mel, mel_len)


def key_mask(cfg, C, Tq, cache_len, chunk_len):
    """[B, Tq, Tk] bool: key j visible to query i (at key position C + i)"""
    Tk = C + Tq
    j = torch.arange(Tk).view(1, 1, Tk)
    ok = (j >= (C - cache_len).view(-1, 1, 1)) & (j < (C + chunk_len).view(-1, 1, 1))
    return ok & R.context_mask(cfg, Tk)[C:, :].unsqueeze(0)


def chunk_attention(P, pfx, cfg, x, kv_in, pos_emb, visible):
    """x [B, Tq, d] (queries), kv_in [B, Tk, d] (keys / values), pos_emb [2Tk-1, d]; score(i, j) uses row j + Tq - 1 - i"""
    B, Tq, d = x.shape
    Tk = kv_in.shape[1]
    H, dk = cfg.n_heads, cfg.d_k
    lin = lambda name, t: F.linear(t, P[pfx + name + ".weight"], P[pfx + name + ".bias"])  # noqa: E731
    q = lin("linear_q", x).view(B, Tq, H, dk)
    k = lin("linear_k", kv_in).view(B, Tk, H, dk).transpose(1, 2)
    v = lin("linear_v", kv_in).view(B, Tk, H, dk).transpose(1, 2)
    p = F.linear(pos_emb, P[pfx + "linear_pos.weight"]).view(2 * Tk - 1, H, dk).transpose(0, 1)
    qu = (q + P[pfx + "pos_bias_u"]).transpose(1, 2)
    qv = (q + P[pfx + "pos_bias_v"]).transpose(1, 2)
    ac = torch.matmul(qu, k.transpose(-2, -1))                         # [B, H, Tq, Tk]
    bd_full = torch.matmul(qv, p.transpose(-2, -1).unsqueeze(0))       # [B, H, Tq, 2Tk-1]
    ii = torch.arange(Tq).unsqueeze(1)
    jj = torch.arange(Tk).unsqueeze(0)
    bd = bd_full[:, :, ii, jj + Tq - 1 - ii]
    scores = (ac + bd) / math.sqrt(dk)
    masked = ~visible.unsqueeze(1)
    attn = torch.softmax(scores.masked_fill(masked, -R.INF_VAL), dim=-1).masked_fill(masked, 0.0)
    ctx = torch.matmul(attn, v).transpose(1, 2).reshape(B, Tq, d)
    return lin("linear_out", ctx)


def conv_module_cached(P, pfx, cfg, x, valid, cache_t):
    """x [B, Tq, d] (normed), cache_t [B, d, K-1] -> (conv module output [B, Tq, d], next time cache)"""
    d, K = cfg.d_model, cfg.conv_kernel
    h = F.linear(x, P[pfx + "pointwise_conv1.weight"].squeeze(-1), P[pfx + "pointwise_conv1.bias"])
    g = h[..., :d] * torch.sigmoid(h[..., d:])
    g = g * valid.unsqueeze(-1).to(g.dtype)
    gt = torch.cat((cache_t, g.transpose(1, 2)), dim=2)                 # [B, d, K-1 + Tq]
    t_next = gt[:, :, gt.shape[2] - (K - 1):]
    c = F.conv1d(gt, P[pfx + "depthwise_conv.weight"], P[pfx + "depthwise_conv.bias"], groups=d)   # [B, d, Tq]
    if cfg.conv_norm_type == "layer_norm":
        c = F.layer_norm(c.transpose(1, 2), (d,), P[pfx + "batch_norm.weight"], P[pfx + "batch_norm.bias"], 1e-5)
        c = c * torch.sigmoid(c)
        return F.linear(c, P[pfx + "pointwise_conv2.weight"].squeeze(-1), P[pfx + "pointwise_conv2.bias"]), t_next
    mean, var = P[pfx + "batch_norm.running_mean"], P[pfx + "batch_norm.running_var"]
    c = (c - mean.view(1, d, 1)) * torch.rsqrt(var.view(1, d, 1) + 1e-5)
    c = c * P[pfx + "batch_norm.weight"].view(1, d, 1) + P[pfx + "batch_norm.bias"].view(1, d, 1)
    c = c * torch.sigmoid(c)
    return F.linear(c.transpose(1, 2), P[pfx + "pointwise_conv2.weight"].squeeze(-1), P[pfx + "pointwise_conv2.bias"]), t_next


def stream_step(P, cfg, mel, mel_len, cache_ch, cache_t, cache_len, drop, subsampling="striding"):
    """one chunk: mel [B, F, pre-encode cache + chunk] -> (out [B, d, Tq], out_len, cache_ch_next, cache_t_next, cache_len_next).
    cfg: R.ConformerCfg with chunked_limited att_context_size, conv_context_size (K-1, 0), causal_downsampling."""
    x, l2 = subsample(P, cfg, mel, mel_len, subsampling)
    T2 = x.shape[1]
    drop = max(0, min(int(drop), T2 - 1))
    x = x[:, drop:]
    B, Tq, d = x.shape
    chunk_len = (l2 - drop).clamp(0, Tq)
    if cfg.xscaling:
        x = x * math.sqrt(d)
    C = cache_ch.shape[2]
    Tk = C + Tq
    cache_len = cache_len.clamp(0, C)
    pos_emb = R.rel_pos_table(Tk, d).to(x.dtype)
    visible = key_mask(cfg, C, Tq, cache_len, chunk_len)
    valid = torch.arange(Tq).unsqueeze(0) < chunk_len.unsqueeze(1)
    ch_next, t_next = [], []
    for l in range(cfg.n_layers):
        pfx = f"layers.{l}."
        r = x + 0.5 * R.feed_forward(P, pfx + "feed_forward1.", cfg, R._ln(P, pfx + "norm_feed_forward1.", x), False)
        y = R._ln(P, pfx + "norm_self_att.", r)
        kv_in = torch.cat((cache_ch[l].to(y.dtype), y), dim=1)
        ch_next.append(kv_in[:, Tk - C:])
        r = r + chunk_attention(P, pfx + "self_attn.", cfg, y, kv_in, pos_emb, visible)
        cv, tn = conv_module_cached(P, pfx + "conv.", cfg, R._ln(P, pfx + "norm_conv.", r), valid, cache_t[l].to(y.dtype))
        t_next.append(tn)
        r = r + cv
        r = r + 0.5 * R.feed_forward(P, pfx + "feed_forward2.", cfg, R._ln(P, pfx + "norm_feed_forward2.", r), False)
        x = R._ln(P, pfx + "norm_out.", r)
    return (x.transpose(1, 2), chunk_len, torch.stack(ch_next), torch.stack(t_next),
            torch.clamp(cache_len + Tq, max=C))


def offline(P, cfg, mel, mel_len, subsampling="striding"):
    """the offline eval forward with the same masks: -> ([B, d, T'], lengths)"""
    if subsampling == "dw_striding":
        from oracle import fastconformer_ref as FC
        return FC.encoder_forward(P, cfg, mel, mel_len)
    return R.encoder_forward(P, cfg, mel, mel_len)
