"""CPU: cache-aware streaming -- the streaming configuration, the initial caches, the chunking buffer, the refusals, and the oracle
of one streaming step (tests/streaming_oracle.py) against the offline oracle in float64: streamed chunk by chunk, a causal encoder
with chunked_limited attention reproduces the offline forward frame for frame."""
import pytest
import torch

from oracle import conformer_ref as R

from streaming_oracle import offline, stream_step


def _enc(**kw):
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    base = dict(feat_in=16, n_layers=2, d_model=32, n_heads=4, conv_kernel_size=5, subsampling="striding", subsampling_factor=4,
                causal_downsampling=True, att_context_size=[8, 3], att_context_style="chunked_limited", conv_context_size="causal",
                dropout=0.0, dropout_pre_encoder=0.0, dropout_emb=0.0, dropout_att=0.0)
    base.update(kw)
    return ConformerEncoder(**base)


@pytest.mark.parametrize("sub,factor,ctx,want", [
    ("striding", 4, [8, 3], dict(chunk_size=[13, 16], shift_size=[13, 16], pre_encode_cache_size=[0, 5], drop_extra_pre_encoded=2,
                                 last_channel_cache_size=8, valid_out_len=4)),
    ("dw_striding", 8, [70, 13], dict(chunk_size=[105, 112], shift_size=[105, 112], pre_encode_cache_size=[0, 9],
                                      drop_extra_pre_encoded=2, last_channel_cache_size=70, valid_out_len=14)),
    ("dw_striding", 8, [70, 0], dict(chunk_size=[1, 8], shift_size=[1, 8], pre_encode_cache_size=[0, 9], drop_extra_pre_encoded=2,
                                     last_channel_cache_size=70, valid_out_len=1)),
])
def test_setup_streaming_params_fields(sub, factor, ctx, want):
    enc = _enc(subsampling=sub, subsampling_factor=factor, conv_kernel_size=9,
               att_context_size=[[70, 13], [70, 6], [70, 1], [70, 0]] if factor == 8 else ctx)
    cfg = enc.setup_streaming_params(att_context_size=ctx)
    assert enc.streaming_cfg is cfg and cfg.cache_drop_size == 0
    for k, v in want.items():
        assert getattr(cfg, k) == v, (k, getattr(cfg, k), v)
    assert cfg.last_channel_num == cfg.last_time_num == enc.n_layers
    ch, tm, ln = enc.get_initial_cache_state(batch_size=3)
    assert tuple(ch.shape) == (2, 3, ctx[0], 32) and ch.dtype == torch.float32 and not ch.any()
    assert tuple(tm.shape) == (2, 3, 32, 8) and tm.dtype == torch.float32 and not tm.any()
    assert tuple(ln.shape) == (3,) and ln.dtype == torch.int64 and not ln.any()


def test_default_context_and_lazy_setup():
    enc = _enc()
    assert enc.streaming_cfg is None
    ch, _, _ = enc.get_initial_cache_state(batch_size=1, dtype=torch.float64)
    assert enc.streaming_cfg.chunk_size == [13, 16] and ch.dtype == torch.float64
    with pytest.raises(ValueError):
        enc.setup_streaming_params(att_context_size=[16, 3])   # not a trained context


def test_buffer_chunks_a_ragged_batch():
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    enc = _enc()
    g = torch.Generator().manual_seed(0)
    T = 90
    mel = torch.randn(3, 16, T, generator=g)
    lens = torch.tensor([90, 61, 12])
    buf = CacheAwareStreamingAudioBuffer(enc, mel, lens)
    chunks = list(buf)
    assert len(chunks) == len(CacheAwareStreamingAudioBuffer(enc, mel, lens)) == 1 + -(-(T - 13) // 16)
    bodies, idx = [], 0
    for k, (c, cl) in enumerate(chunks):
        pre = 0 if k == 0 else 5
        body = 13 if k == 0 else 16
        width = min(pre + body, pre + T - idx)
        assert tuple(c.shape) == (3, 16, width)
        assert torch.equal(c[:, :, :pre], mel[:, :, idx - pre: idx])   # the previous input's last frames
        assert torch.equal(cl, torch.clamp(lens - (idx - pre), 0, width))
        bodies.append(c[:, :, pre:])
        idx += body
    assert torch.equal(torch.cat(bodies, dim=-1), mel)


@pytest.mark.parametrize("kw,match", [
    (dict(att_context_style="regular"), "att_context_style"),
    (dict(conv_context_size=None), "conv_context_size"),
    (dict(conv_context_size=[2, 2]), "conv_context_size"),
    (dict(causal_downsampling=False), "causal_downsampling"),
    (dict(att_context_size=[-1, 3]), "unlimited left"),
])
def test_streaming_refusals(kw, match):
    enc = _enc(**kw)
    with pytest.raises(NotImplementedError, match=match):
        enc.setup_streaming_params()


def test_streaming_refuses_explicit_chunking_and_training_mode():
    enc = _enc()
    with pytest.raises(NotImplementedError, match="chunk_size"):
        enc.setup_streaming_params(chunk_size=16)
    with pytest.raises(NotImplementedError, match="shift_size"):
        enc.setup_streaming_params(shift_size=16)
    ch, tm, ln = enc.get_initial_cache_state(batch_size=1)
    enc.train()
    with pytest.raises(RuntimeError, match="training"):
        enc.cache_aware_stream_step(processed_signal=torch.zeros(1, 16, 13), processed_signal_length=torch.tensor([13]),
                                    cache_last_channel=ch, cache_last_time=tm, cache_last_channel_len=ln)


def _f64_params(enc, seed):
    g = torch.Generator().manual_seed(seed)
    P = {k: v.detach().clone().to(torch.float64) for k, v in enc.state_dict().items()}
    for k in list(P):
        if k.endswith("running_mean"):
            P[k] = 0.2 * torch.randn(P[k].shape, generator=g, dtype=torch.float64)
        elif k.endswith("running_var"):
            P[k] = 0.5 + torch.rand(P[k].shape, generator=g, dtype=torch.float64)
        elif k.endswith(("pos_bias_u", "pos_bias_v")) or "norm" in k and k.endswith(("weight", "bias")):
            P[k] = P[k] + 0.1 * torch.randn(P[k].shape, generator=g, dtype=torch.float64)
    return P


def stream_all(P, cfg, enc, mel, lens, sub):
    """streams a whole batch through the oracle step; -> per utterance the concatenated valid output frames [d, n_b]"""
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    ch, tm, ln = enc.get_initial_cache_state(batch_size=mel.shape[0], dtype=mel.dtype)
    outs = [[] for _ in range(mel.shape[0])]
    n_chunks = 0
    buf = CacheAwareStreamingAudioBuffer(enc, mel, lens)
    for chunk, cl in buf:
        drop = buf.drop_extra_pre_encoded
        o, ol, ch, tm, ln = stream_step(P, cfg, chunk, cl, ch, tm, ln, drop, subsampling=sub)
        for b in range(mel.shape[0]):
            outs[b].append(o[b, :, : int(ol[b])])
        n_chunks += 1
    return [torch.cat(o, dim=1) for o in outs], n_chunks


@pytest.mark.parametrize("ctx", [[8, 3], [8, 0]])
@pytest.mark.parametrize("norm", ["batch_norm", "layer_norm"])
def test_streaming_oracle_equals_offline_oracle_in_float64(norm, ctx):
    """x4 causal encoder, [8, 3] (8 chunks: the channel cache fills after two and then rolls over) and [8, 0] (one-frame chunks,
    the second one behind a pre-encode cache cut at frame 0), K = 5, ragged B = 3: the concatenation of the streamed chunks equals
    the offline forward with the same chunked_limited mask on every valid frame"""
    enc = _enc(conv_norm_type=norm, att_context_size=ctx)
    P = _f64_params(enc, 1)
    cfg = R.ConformerCfg(feat_in=16, d_model=32, n_heads=4, n_layers=2, conv_kernel=5, att_context_size=tuple(ctx),
                         att_context_style="chunked_limited", conv_norm_type=norm, conv_context_size=(4, 0),
                         causal_downsampling=True, dropout=0.0, dropout_att=0.0, dropout_pre_encoder=0.0)
    g = torch.Generator().manual_seed(2)
    T = 120
    mel = torch.randn(3, 16, T, generator=g, dtype=torch.float64)
    lens = torch.tensor([120, 97, 58])
    ref, ref_len = offline(P, cfg, mel, lens)
    enc.setup_streaming_params()
    got, n_chunks = stream_all(P, cfg, enc, mel, lens, "striding")
    assert n_chunks >= 6
    for b in range(3):
        n = int(ref_len[b])
        assert got[b].shape[1] == n, (b, got[b].shape, n)
        err = (got[b] - ref[b, :, :n]).abs().max().item()
        assert err < 1e-10, (b, err)


def test_buffer_cuts_a_pre_encode_cache_that_reaches_before_the_stream():
    """lookahead 0 ([8, 0], x4: chunks [1, 4], cache 5): the second chunk has one frame in front of it -- the cache is that one
    frame, and the drop is the one output frame the first chunk produced already"""
    from nemo_amd.streaming import CacheAwareStreamingAudioBuffer
    enc = _enc(att_context_size=[8, 0])
    mel = torch.randn(2, 16, 20)
    buf = CacheAwareStreamingAudioBuffer(enc, mel, torch.tensor([20, 7]))
    it = iter(buf)
    c0, _ = next(it)
    assert c0.shape[-1] == 1 and buf.drop_extra_pre_encoded == 0
    c1, l1 = next(it)
    assert torch.equal(c1, mel[:, :, :5]) and buf.drop_extra_pre_encoded == 1 and torch.equal(l1, torch.tensor([5, 5]))
    c2, l2 = next(it)
    assert torch.equal(c2, mel[:, :, 0:9]) and buf.drop_extra_pre_encoded == 2 and torch.equal(l2, torch.tensor([9, 7]))
