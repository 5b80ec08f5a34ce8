"""-m gpu: ConformerEncoder with a limited attention context on the windowed fused kernels (use_flash_ctx_attention): parity with
the GEMM + softmax path below its 1024-frame limit, and a forward + backward above it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
CONTEXTS = [dict(att_context_size=[70, 13], att_context_style="chunked_limited"),
            dict(att_context_size=[16, 16], self_attention_model="rel_pos_local_attn")]
IDS = ["chunked_limited_70_13", "local_attn_16_16"]


def _encoder(cdt, ctx, flash_ctx=None):
    from nemo_amd.modules.conformer_encoder import ConformerEncoder
    enc = ConformerEncoder(feat_in=80, n_layers=1, d_model=128, n_heads=2, conv_kernel_size=9, dropout=0.0, dropout_pre_encoder=0.0,
                           dropout_emb=0.0, dropout_att=0.0, compute_dtype=cdt, **ctx)
    enc.use_flash_ctx_attention = flash_ctx
    return enc.to(dev).train()


def _run(enc, x, n):
    y, yl = enc(audio_signal=x, length=n)
    (y.float() ** 2).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().float().cpu() for k, p in enc.named_parameters() if k.startswith("layers.") and p.grad is not None}
    return y.detach().float().cpu(), yl.cpu(), grads


@pytest.mark.parametrize("ctx", CONTEXTS, ids=IDS)
def test_windowed_path_follows_fp32_as_closely_as_the_gemm_path(ctx):
    """about 200 encoder frames, ragged lengths: relative error (output and every layer parameter's gradient, sum-of-squares loss)
    of the windowed path against the fp32 encoder <= 2 x that of the existing bf16 path, measured here (another, equally
    legitimate rounding order)"""
    torch.manual_seed(11)
    e32 = _encoder(torch.float32, ctx)
    x = torch.randn(3, 80, 803, generator=torch.Generator().manual_seed(12)).to(dev)
    n = torch.tensor([803, 531, 90]).to(dev)
    runs = {}
    for name, cdt, flag in (("fp32", torch.float32, None), ("gemm", torch.bfloat16, False), ("windowed", torch.bfloat16, True)):
        enc = e32 if name == "fp32" else _encoder(cdt, ctx, flag)
        enc.load_state_dict(e32.state_dict())
        assert enc._ctx_limited_any() and not enc._flash_ok()
        runs[name] = _run(enc, x, n)
    y32, yl32, g32 = runs["fp32"]
    assert len(g32) > 20 and torch.equal(runs["windowed"][1], yl32) and torch.equal(runs["gemm"][1], yl32)
    rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-30)).item()  # noqa: E731
    worst = 0.0
    for k in ["output"] + sorted(g32):
        ref = y32 if k == "output" else g32[k]
        eg = rel(runs["gemm"][0] if k == "output" else runs["gemm"][2][k], ref)
        ew = rel(runs["windowed"][0] if k == "output" else runs["windowed"][2][k], ref)
        worst = max(worst, ew / max(eg, 1e-30))
        print(f"{k}: relative error against fp32 -- GEMM + softmax path {eg:.3e}, windowed kernels {ew:.3e}")
        assert ew <= 2 * eg, (k, ew, eg)
    print(f"worst windowed / gemm error ratio {worst:.3f}")


@pytest.mark.parametrize("ctx", CONTEXTS, ids=IDS)
def test_default_encoder_runs_above_1024_frames(ctx):
    """1050 encoder frames with the attribute at its default: the soft-max kernel's path refuses, the windowed kernels run"""
    torch.manual_seed(13)
    enc = _encoder(torch.bfloat16, ctx)
    assert enc.use_flash_ctx_attention is None
    x = torch.randn(2, 80, 4197, generator=torch.Generator().manual_seed(14)).to(dev)
    n = torch.tensor([4197, 3001]).to(dev)
    y, yl, grads = _run(enc, x, n)
    assert y.shape[-1] == 1050 and yl.tolist() == [1050, 751]
    assert torch.isfinite(y).all() and len(grads) > 20 and all(torch.isfinite(g).all() for g in grads.values())
