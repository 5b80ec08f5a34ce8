"""-m gpu: cache-aware streaming on the HIP path -- the chunk-attention and cached depthwise-conv kernels against torch, one encoder
step against the streaming oracle (tests/streaming_oracle.py), streaming against the offline forward in fp32 and bf16, and the CTC
model's conformer_stream_step against offline greedy decoding."""
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import conformer_ref as R

import streaming_oracle as SO

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16_SLACK = 2.5   # the repo's factor over what bf16 rounding at the storage points explains (test_baseline_configs_gpu.py)


def _enc(compute_dtype=torch.float32, **kw):
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    base = dict(feat_in=16, n_layers=2, d_model=32, n_heads=4, conv_kernel_size=5, subsampling="striding", subsampling_factor=4,
                causal_downsampling=True, att_context_size=[8, 3], att_context_style="chunked_limited", conv_context_size="causal",
                dropout=0.0, dropout_pre_encoder=0.0, dropout_emb=0.0, dropout_att=0.0, compute_dtype=compute_dtype)
    base.update(kw)
    return ConformerEncoder(**base)


def _randomise(enc, seed):
    """non-trivial BatchNorm statistics, LayerNorm affine and positional biases (the defaults are 0 / 1)"""
    g = torch.Generator().manual_seed(seed)
    sd = enc.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif k.endswith(("pos_bias_u", "pos_bias_v")) or ("norm" in k and k.endswith(("weight", "bias"))):
            v.add_(0.1 * torch.randn(v.shape, generator=g))
    enc.load_state_dict(sd)
    return enc


# ------------------------------------------------------------------------------------------------ kernels
def _attn_ref(q, kv, pos, bu, bv, cache_len, chunk_len, B, H, Tq, Tk, dk, dA, chunk, left_chunks, scale, dt):
    """float64 reference from the same operands (q + u, q + v rounded to the operand dtype, as the kernel and the offline path)"""
    C = Tk - Tq
    qf = q.double().view(B, Tq, H, dk)
    rnd = lambda t: t.to(dt).double()   # noqa: E731
    qu = rnd(qf + bu.double().view(H, dk)).transpose(1, 2)
    qv = rnd(qf + bv.double().view(H, dk)).transpose(1, 2)
    k = kv[:, :dA].double().view(B, Tk, H, dk).transpose(1, 2)
    v = kv[:, dA:].double().view(B, Tk, H, dk).transpose(1, 2)
    p = pos.double().view(2 * Tk - 1, H, dk).transpose(0, 1)
    ii = torch.arange(Tq, device=q.device).view(-1, 1)
    jj = torch.arange(Tk, device=q.device).view(1, -1)
    s = (qu @ k.transpose(-1, -2) + (qv @ p.transpose(-1, -2).unsqueeze(0))[:, :, ii, jj + Tq - 1 - ii]) * scale
    vis = (jj >= (C - cache_len).view(-1, 1, 1)) & (jj < (C + chunk_len).view(-1, 1, 1))
    if chunk > 0:
        dc = torch.div(C + ii, chunk, rounding_mode="floor") - torch.div(jj, chunk, rounding_mode="floor")
        ok = dc >= 0
        if left_chunks >= 0:
            ok = ok & (dc <= left_chunks)
        vis = vis & ok
    vis = vis.unsqueeze(1)
    a = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1).nan_to_num(0.0).masked_fill(~vis, 0.0)
    return (a @ v).transpose(1, 2).reshape(B * Tq, dA)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dk,H,Tq,C,chunk,left_chunks", [
    (64, 8, 14, 70, 14, 5),     # the recipe's [70, 13] step
    (128, 4, 14, 70, 14, 5),
    (48, 4, 4, 8, 4, 2),        # a padded head width ([8, 3])
    (12, 2, 5, 0, 0, -1),       # C = 0, no chunk rule, an odd width
    (64, 2, 3, 40, 2, -1),      # Tq not a multiple of the chunk, unlimited left chunks
])
def test_stream_attention_kernel_against_torch(dt, dk, H, Tq, C, chunk, left_chunks):
    from nemo_amd import ops
    g = torch.Generator().manual_seed(dk * 100 + Tq + C)
    B, Tk, dA = 5, C + Tq, H * dk
    q = torch.randn(B * Tq, dA, generator=g).to(dev, dt)
    kv = torch.randn(B * Tk, 2 * dA, generator=g).to(dev, dt)
    pos = torch.randn(2 * Tk - 1, dA, generator=g).to(dev, dt)
    bu, bv = (0.3 * torch.randn(dA, generator=g)).to(dev), (0.3 * torch.randn(dA, generator=g)).to(dev)
    cache_len = torch.tensor([0, C, C // 2, C, max(C - 3, 0)], dtype=torch.int64).to(dev)        # empty, full, partial
    chunk_len = torch.tensor([Tq, Tq, Tq - 1, 0, 1], dtype=torch.int64).to(dev)                   # ragged, including 0
    scale = 1.0 / math.sqrt(dk)
    ctx = torch.full((B * Tq, dA), float("nan"), device=dev).to(dt)
    ops.stream_attn(q, dA, kv, 2 * dA, dA, pos, dA, bu, bv, cache_len, chunk_len, ctx, dA, B, H, Tq, Tk, dk, scale,
                    chunk=chunk, left_chunks=left_chunks)
    torch.cuda.synchronize()
    ref = _attn_ref(q, kv, pos, bu, bv, cache_len, chunk_len, B, H, Tq, Tk, dk, dA, chunk, left_chunks, scale, dt)
    got = ctx.double()
    assert torch.isfinite(got).all()
    # f32: accumulation-order noise; bf16: the output is stored as bf16 (half an ulp = 2^-9 relative) -> one ulp of slack
    tol = (2e-5 if dt == torch.float32 else 2.0 ** -8) * ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert err <= tol, (err, tol)
    if C > 0:   # utterance 3: no chunk frames and a full cache -- every query still sees the cache
        assert got.view(B, Tq, dA)[3].abs().max() > 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K", [3, 5, 9, 31])
@pytest.mark.parametrize("Tq", [1, 4, 14])
def test_stream_dwconv_kernel_against_conv1d_on_the_concatenation(dt, K, Tq):
    from nemo_amd import ops
    g = torch.Generator().manual_seed(K * 10 + Tq)
    B, d = 3, 72
    x = torch.randn(B * Tq, d, generator=g).to(dev, dt)
    cache = torch.randn(B, d, K - 1, generator=g).to(dev)
    w = torch.randn(d, 1, K, generator=g).to(dev) / math.sqrt(K)
    b = torch.randn(d, generator=g).to(dev)
    y = torch.empty(B * Tq, d, device=dev, dtype=dt)
    nxt = torch.full((B, d, K - 1), float("nan"), device=dev)
    cache0 = cache.clone()
    ops.stream_dwconv(x, cache, w, b, y, nxt, B, Tq, d, K)
    torch.cuda.synchronize()
    full = torch.cat((cache.double(), x.double().view(B, Tq, d).transpose(1, 2)), dim=2)       # [B, d, K-1+Tq]
    ref = F.conv1d(full, w.double(), b.double(), groups=d).transpose(1, 2).reshape(B * Tq, d)
    tol = (1e-5 if dt == torch.float32 else 2.0 ** -8) * ref.abs().max().item()
    assert (y.double() - ref).abs().max().item() <= tol
    assert torch.equal(nxt, full[:, :, full.shape[2] - (K - 1):].float())      # (exact: copies of f32 / bf16 values)
    assert torch.equal(cache, cache0)


# ------------------------------------------------------------------------------------------------ one encoder step
def _cfg(enc, **kw):
    return R.ConformerCfg(feat_in=enc._feat_in, d_model=enc.d_model, n_heads=enc.n_heads, n_layers=enc.n_layers,
                          conv_kernel=enc.conv_kernel_size, att_context_size=tuple(enc.att_context_size),
                          att_context_style="chunked_limited", conv_norm_type=enc.conv_norm_type,
                          conv_context_size=(enc.conv_kernel_size - 1, 0), causal_downsampling=True, dropout=0.0, dropout_att=0.0,
                          dropout_pre_encoder=0.0, conv_channels=enc.pre_encode._conv_channels, **kw)


@pytest.mark.parametrize("norm", ["batch_norm", "layer_norm"])
def test_one_encoder_step_against_the_streaming_oracle(norm):
    enc = _randomise(_enc(conv_norm_type=norm), 3).to(dev).eval()
    P = {k: v.detach().double().cpu() for k, v in enc.state_dict().items()}
    cfg = _cfg(enc)
    g = torch.Generator().manual_seed(4)
    B, d = 3, 32
    enc.setup_streaming_params()
    ch = torch.randn(2, B, 8, d, generator=g)
    tm = torch.randn(2, B, d, 4, generator=g)
    ln = torch.tensor([0, 4, 8])
    mel = torch.randn(B, 16, 21, generator=g)
    ml = torch.tensor([21, 14, 5])
    ins = [t.to(dev) for t in (ch, tm, ln)]
    keep = [t.clone() for t in ins]
    o, ol, chn, tmn, lnn = enc.cache_aware_stream_step(processed_signal=mel.to(dev), processed_signal_length=ml.to(dev),
                                                       cache_last_channel=ins[0], cache_last_time=ins[1], cache_last_channel_len=ins[2])
    torch.cuda.synchronize()
    for a, b in zip(ins, keep):
        assert torch.equal(a, b)   # the input caches are not modified
    ro, rol, rch, rtm, rln = SO.stream_step(P, cfg, mel.double(), ml, ch.double(), tm.double(), ln, 2, "striding")
    assert torch.equal(ol.cpu(), rol) and torch.equal(lnn.cpu(), rln)
    for got, ref, what in ((o, ro, "out"), (chn, rch, "cache_last_channel"), (tmn, rtm, "cache_last_time")):
        got = got.double().cpu()
        if what == "out":   # valid frames only (padded frames are not part of the contract)
            got = torch.cat([got[b, :, : int(rol[b])] for b in range(B)], dim=1)
            ref = torch.cat([ref[b, :, : int(rol[b])] for b in range(B)], dim=1)
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        assert err < 1e-5, (what, err)


# ------------------------------------------------------------------------------------------------ streaming == offline
def _stream_all(enc, mel, lens):
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    ch, tm, ln = enc.get_initial_cache_state(batch_size=mel.shape[0])
    outs = [[] for _ in range(mel.shape[0])]
    n = 0
    buf = CacheAwareStreamingAudioBuffer(enc, mel, lens)
    for chunk, cl in buf:
        o, ol, ch2, tm2, ln2 = enc.cache_aware_stream_step(processed_signal=chunk, processed_signal_length=cl, cache_last_channel=ch,
                                                           cache_last_time=tm, cache_last_channel_len=ln,
                                                           drop_extra_pre_encoded=buf.drop_extra_pre_encoded)
        assert ch2.data_ptr() != ch.data_ptr() and tm2.data_ptr() != tm.data_ptr() and ln2.data_ptr() != ln.data_ptr()
        ch, tm, ln = ch2, tm2, ln2
        ol = ol.cpu()
        for b in range(mel.shape[0]):
            outs[b].append(o[b, :, : int(ol[b])].float())
        n += 1
    return [torch.cat(o, dim=1) for o in outs], n


@pytest.mark.parametrize("sub,factor", [("striding", 4), ("dw_striding", 8)])
@pytest.mark.parametrize("ctx", [[8, 3], [8, 0]])
@pytest.mark.parametrize("norm", ["batch_norm", "layer_norm"])
def test_streaming_equals_offline_fp32(sub, factor, ctx, norm):
    enc = _randomise(_enc(subsampling=sub, subsampling_factor=factor, att_context_size=ctx, conv_norm_type=norm,
                          feat_in=32), 5).to(dev).eval()
    enc.setup_streaming_params()
    g = torch.Generator().manual_seed(6)
    shift = enc.streaming_cfg.shift_size[1]
    T = enc.streaming_cfg.chunk_size[0] + max(6, -(-160 // shift)) * shift   # >= 6 chunks, >= 160 frames
    mel = torch.randn(3, 32, T, generator=g).to(dev)
    lens = torch.tensor([T, T - 37, T // 2]).to(dev)
    with torch.no_grad():
        ref, ref_len = enc(audio_signal=mel, length=lens)
    got, n = _stream_all(enc, mel, lens)
    torch.cuda.synchronize()
    assert n >= 6
    for b in range(3):
        L = int(ref_len[b])
        assert got[b].shape[1] == L, (b, got[b].shape, L)
        r = ref[b, :, :L]
        per_frame = (got[b] - r).norm(dim=0) / r.norm(dim=0).clamp_min(1e-12)
        assert per_frame.max().item() <= 1e-5, (b, per_frame.max().item())


def test_streaming_equals_offline_bf16_recipe_geometry():
    """the cache-aware FastConformer recipe's layer geometry (d_model 512, 8 heads, K 9, dw_striding x8 with 256 channels,
    [70, 13], LayerNorm conv module), 2 layers, bf16: streamed may not sit farther from the fp32 truth than BF16_SLACK x what bf16
    rounding at the storage points explains (the oracle with emulate_bf16)"""
    kw = dict(feat_in=80, n_layers=2, d_model=512, n_heads=8, conv_kernel_size=9, subsampling="dw_striding", subsampling_factor=8,
              subsampling_conv_channels=256, att_context_size=[70, 13], conv_norm_type="layer_norm")
    torch.manual_seed(7)
    e32 = _randomise(_enc(torch.float32, **kw), 8)
    e16 = _enc(torch.bfloat16, **kw)
    e16.load_state_dict(e32.state_dict())
    P = {k: v.detach().float().cpu() for k, v in e32.state_dict().items()}
    e32, e16 = e32.to(dev).eval(), e16.to(dev).eval()
    g = torch.Generator().manual_seed(9)
    T = 105 + 5 * 112 + 40
    mel = torch.randn(2, 80, T, generator=g)
    lens = torch.tensor([T, T - 211])
    from oracle import fastconformer_ref as FC
    cfg = _cfg(e32)
    with torch.no_grad():
        o32, l32 = FC.encoder_forward(P, cfg, mel, lens)
        oemu, _ = FC.encoder_forward(P, dataclasses.replace(cfg, emulate_bf16=True), mel, lens)
        off16, _ = e16(audio_signal=mel.to(dev), length=lens.to(dev))
    got, n = _stream_all(e16, mel.to(dev), lens.to(dev))
    torch.cuda.synchronize()
    assert n >= 6
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()   # noqa: E731
    for b in range(2):
        L = int(l32[b])
        assert got[b].shape[1] == L
        ref = o32[b, :, :L]
        e_stream, e_emu, e_off = rel(got[b].cpu(), ref), rel(oemu[b, :, :L], ref), rel(off16[b, :, :L].float().cpu(), ref)
        assert e_stream <= BF16_SLACK * e_emu + 5e-3, (b, e_stream, e_emu, e_off)


# ------------------------------------------------------------------------------------------------ model
def test_ctc_conformer_stream_step_matches_offline_greedy():
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    vocab = [chr(ord("a") + i) for i in range(20)]
    cfg = conformer_ctc_config("small", vocab_size=len(vocab), d_model=64, n_heads=4, n_layers=2, subsampling="striding",
                               subsampling_factor=4, causal_downsampling=True, att_context_size=[16, 3],
                               att_context_style="chunked_limited", conv_kernel_size=9, conv_context_size="causal",
                               dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0, compute_dtype=torch.float32)
    cfg["decoder"]["vocabulary"] = vocab
    cfg["preprocessor"]["dither"] = 0.0
    torch.manual_seed(11)
    m = EncDecCTCModel(cfg)
    _randomise(m.encoder, 12)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(13)
    audio = (0.1 * torch.randn(3, 24000, generator=g)).to(dev)
    alen = torch.tensor([24000, 17000, 9000]).to(dev)
    with torch.no_grad():
        mel, mel_len = m.preprocessor(input_signal=audio, length=alen)
        lp, enc_len, _ = m.forward(processed_signal=mel, processed_signal_length=mel_len)
    enc = m.encoder
    ch, tm, ln = enc.get_initial_cache_state(batch_size=3)
    prev = None
    buf = CacheAwareStreamingAudioBuffer(m, mel, mel_len)
    for chunk, cl in buf:
        res = m.conformer_stream_step(processed_signal=chunk, processed_signal_length=cl, cache_last_channel=ch, cache_last_time=tm,
                                      cache_last_channel_len=ln, previous_pred_out=prev, drop_extra_pre_encoded=buf.drop_extra_pre_encoded,
                                      return_transcription=True, return_log_probs=True)
        preds, texts, ch2, tm2, ln2, best, slp, slen = res
        assert best is None and len(texts) == 3
        for a, b in ((ch, ch2), (tm, tm2), (ln, ln2)):
            assert a.data_ptr() != b.data_ptr()
        ch, tm, ln, prev = ch2, tm2, ln2, preds
    torch.cuda.synchronize()
    top2 = lp.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]).cpu()
    off_pred = lp.argmax(-1).cpu()
    blank = len(vocab)
    for b in range(3):
        L = int(enc_len[b])
        assert prev[b].numel() == L and int(slen[b]) == L
        diff = (prev[b] != off_pred[b, :L]) & (margin[b, :L] >= 1e-4)
        assert not diff.any(), (b, diff.nonzero())
        ids = [int(t) for t in torch.unique_consecutive(off_pred[b, :L]).tolist() if int(t) != blank]
        if torch.equal(prev[b], off_pred[b, :L]):
            assert texts[b] == "".join(vocab[i] for i in ids)


def test_rnnt_conformer_stream_step_is_refused():
    from nemo_amd.models import EncDecRNNTModel
    with pytest.raises(NotImplementedError, match="partial_hypotheses"):
        EncDecRNNTModel.conformer_stream_step(None)
