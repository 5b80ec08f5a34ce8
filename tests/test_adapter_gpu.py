"""-m gpu: the fused linear-adapter kernels (csrc/adapter.hip) against a float64 restatement of the rule in include/mi355x_asr.h, and
the adapter wiring of ConformerEncoder / EncDecCTCModel against oracle/conformer_ref.py in float64.

Tolerance per tensor (the project's rule): the restatement run at the kernel's precision (float32; bf16: the four operands rounded)
has its own max error against float64 on the case; allowed is max(8 x that error, 16 ulp of the tensor's largest magnitude)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"


def _rule(x, g, b, wd, wu, dt, rnd=None):
    """y = x + W_up . swish(W_down . LayerNorm(x)) in `dt`; rnd: rounding of the operands n, a (and, through autograd, of nothing else)"""
    q = (lambda t: t + (t.detach().to(rnd).to(dt) - t.detach())) if rnd else (lambda t: t)   # value rounded, gradient straight through
    x, g, b, wd, wu = (t.to(dt) for t in (x, g, b, wd, wu))
    n = torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, 1e-5)
    h = q(n) @ q(wd).t()
    a = h * torch.sigmoid(h)
    return x + q(a) @ q(wu).t()


def _bwd_rule(x, dy, g, b, wd, wu, dt, rnd=None):
    """(y, dx, dWd, dWu, dg, db) of the rule in `dt`; with `rnd` the backward's dy and dh operands are rounded too, as the rule says"""
    q = (lambda t: t.to(rnd).to(dt)) if rnd else (lambda t: t)
    x, dy, g, b, wd, wu = (t.to(dt) for t in (x, dy, g, b, wd, wu))
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, g, b))
    n = torch.nn.functional.layer_norm(xr, (x.shape[-1],), gr, br, 1e-5)
    nq, wdq, wuq = q(n.detach()), q(wd), q(wu)
    h = nq @ wdq.t()
    s = torch.sigmoid(h)
    a = h * s
    y = x + q(a) @ wuq.t()
    dyq = q(dy)
    dh = q((dyq @ wuq) * (s * (1 + h * (1 - s))))
    dn = dh @ wdq
    n.backward(dn)
    return y, dy + xr.grad, dh.t() @ nq, dyq.t() @ q(a), gr.grad, br.grad


def _case(M, d, dim, seed=0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x = r(M, d) * (0.5 + r(M, 1).abs()) + 2.0 * r(M, 1)      # per-row scale and offset: the LayerNorm matters
    return x, r(M, d), 1.0 + 0.3 * r(d), 0.2 * r(d), r(dim, d) / d ** 0.5, r(d, dim) / dim ** 0.5


def _check(names, got, ref, low):
    bad = []
    for k, g_, r_, l_ in zip(names, got, ref, low):
        err = (g_.double().cpu() - r_).abs().max().item()
        bound = max(8 * (l_.double() - r_).abs().max().item(), 16 * float(np.spacing(np.float32(r_.abs().max().item()))))
        print(f"{k}: err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


def _run(M, d, dim, cdt, pitch=0, prefill=0.0):
    from nemo_amd import ops
    x, dy, g, b, wd, wu = _case(M, d, dim)
    rnd = torch.bfloat16 if cdt == torch.bfloat16 else None
    ref = _bwd_rule(x, dy, g, b, wd, wu, torch.float64)
    low = _bwd_rule(x, dy, g, b, wd, wu, torch.float32, rnd)
    ld = d + pitch
    xd, dyd = (torch.zeros(M, ld, device=dev).copy_(torch.nn.functional.pad(t.float(), (0, pitch))) for t in (x, dy))
    gd, bd = g.float().to(dev), b.float().to(dev)
    wdd, wud = wd.to(cdt).to(dev).contiguous(), wu.to(cdt).to(dev).contiguous()
    y, dx = torch.empty(M, ld, device=dev), torch.empty(M, ld, device=dev)
    ops.adapter_fwd(xd, gd, bd, wdd, wud, y, M, d, dim, ldx=ld, ldy=ld)
    grads = [torch.full(s, prefill, device=dev) for s in ((dim, d), (d, dim), (d,), (d,))]
    ws = torch.empty(ops.adapter_workspace_bytes(M, d, dim, cdt), dtype=torch.uint8, device=dev)
    ops.adapter_bwd(xd, dyd, gd, bd, wdd, wud.t().contiguous(), wdd.t().contiguous(), dx, *grads, ws, M, d, dim, ldx=ld, lddy=ld, lddx=ld)
    torch.cuda.synchronize()
    return [y[:, :d], dx[:, :d]] + [t - prefill for t in grads], ref, low


NAMES = ("y", "dx", "dW_down", "dW_up", "dgamma", "dbeta")


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,d,dim,pitch,prefill", [(1, 64, 8, 0, 0.0), (37, 176, 24, 8, 0.0), (1000, 512, 32, 0, 0.5), (300, 1024, 64, 0, 0.0)])
def test_kernels_match_float64(M, d, dim, pitch, prefill, cdt):
    got, ref, low = _run(M, d, dim, cdt, pitch, prefill)
    _check(NAMES, got, ref, low)


def test_backward_is_deterministic():
    a, _, _ = _run(1000, 512, 32, torch.bfloat16)
    b, _, _ = _run(1000, 512, 32, torch.bfloat16)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_entry_refuses_before_launching():
    from nemo_amd._lib import lib
    t = torch.zeros(64 * 256, device=dev)
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream

    def bwd(d, dim, dtype, ws_bytes, x=p):
        return lib.mi355x_adapter_bwd(x, d, p, d, p, p, p, d, p, d, p, dim, p, d, p, p, p, p, p, ws_bytes, 4, d, dim, dtype, 1e-5, st)
    big = 1 << 30
    assert bwd(64, 12, 0, big) == 1 and bwd(64, 136, 0, big) == 1 and bwd(180, 8, 1, big) == 1
    assert bwd(64, 8, 0, lib.mi355x_adapter_workspace_bytes(4, 64, 8, 0) - 1) == 1 and bwd(64, 8, 0, big, x=None) == 1
    assert lib.mi355x_adapter_fwd(p, 64, p, p, p, 64, p, 12, p, 64, 4, 64, 12, 0, 1e-5, st) == 1
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ model wiring
CFG = dict(in_features=32, dim=8, activation="swish", norm_position="pre", dropout=0.0)


def _model(seed=5, d_model=32, cdt=torch.float32):
    from oracle import conformer_ref as R
    from nemo_amd.models import EncDecCTCModel, conformer_ctc_config
    over = dict(d_model=d_model, n_heads=d_model // 8 if d_model < 512 else 8, n_layers=2, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0)
    cfg = conformer_ctc_config("small", vocab_size=16, **over)
    cfg["preprocessor"]["dither"] = 0.0
    model = EncDecCTCModel(cfg)
    model.encoder.compute_dtype = model.decoder.compute_dtype = cdt
    P = R.init_params(R.ConformerCfg(vocab=16, **over), seed=seed)
    model.load_state_dict({k: v.clone() for k, v in P.items() if k.startswith(("encoder.", "decoder."))}, strict=False)
    return model.to(dev), P, R.ConformerCfg(vocab=16, **over)


def _randomise(model, seed=3):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".adapter_layer." in n:
                p.copy_((0.3 * torch.randn(p.shape, generator=gen) + (1.0 if n.endswith("module.0.weight") else 0.0)).to(dev))
    model.encoder.weights_updated()


def _batch():
    from oracle import conformer_ref as R
    audio, _, tok, _ = R.synthetic_batch(3, 1.3, vocab=16, seed=99)
    return audio, torch.tensor([20800, 15000, 7777]), tok, torch.tensor([3, 2, 3])


def _enc(model, audio, alen):
    with torch.no_grad():
        mel, ml = model.preprocessor(input_signal=audio.to(dev), length=alen.to(dev))
        return model.encoder(audio_signal=mel, length=ml)[0]


def test_zero_initialised_and_disabled_adapters_change_nothing(tmp_path):
    model, _, _ = _model()
    model.eval()
    audio, alen, _, _ = _batch()
    base = _enc(model, audio, alen)
    model.add_adapter("a", dict(CFG))
    assert torch.equal(_enc(model, audio, alen), base)
    _randomise(model)
    adapted = _enc(model, audio, alen)
    assert not torch.equal(adapted, base)
    model.set_enabled_adapters(enabled=False)
    assert model.get_enabled_adapters() == [] and torch.equal(_enc(model, audio, alen), base)
    # save / load into a fresh model with the same base weights: identical bits
    model.set_enabled_adapters("encoder:a", True)
    model.save_adapters(str(tmp_path / "a.pt"))
    fresh, _, _ = _model()
    fresh.eval()
    fresh.load_adapters(str(tmp_path / "a.pt"))
    assert fresh.get_enabled_adapters() == ["a"] and torch.equal(_enc(fresh, audio, alen), adapted)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_adapted_model_matches_oracle(monkeypatch, packed):
    """encoder output (valid frames) and the CTC-loss gradients of every adapter parameter against the oracle in float64 with the
    adapter restatement in front of each norm_out; ragged batch, through the padded and the packed-rows path"""
    from oracle import conformer_ref as R
    model, P, cfg = _model()
    model.add_adapter("a", dict(CFG))
    _randomise(model)
    model.encoder.packed_rows = packed
    model.train()
    audio, alen, tok, tl = _batch()
    ad = {"encoder." + n: p.detach().cpu() for n, p in model.encoder.named_parameters() if ".adapter_layer." in n}
    ln = R._ln

    def run(dt):
        Q = {k: v.to(dt) if v.is_floating_point() else v for k, v in {**P, **ad}.items()}
        Q.update({k: Q[k].clone().requires_grad_(True) for k in ad})

        def ln_ad(P_, pfx, x):
            if pfx.endswith("norm_out."):
                a = pfx[:-len("norm_out.")] + "adapter_layer.a.module."
                x = _rule(x, Q[a + "0.weight"], Q[a + "0.bias"], Q[a + "1.weight"], Q[a + "3.weight"], dt)
            return ln(P_, pfx, x)
        monkeypatch.setattr(R, "_ln", ln_ad)
        mel, mel_len = R.log_mel_features(audio, alen, fb=P.get("preprocessor.featurizer.fb"), window=P.get("preprocessor.featurizer.window"),
                                          n_mels=cfg.feat_in)   # (model_forward's own steps, the features cast to `dt`)
        enc, enc_len = R.encoder_forward(Q, cfg, mel.to(dt), mel_len, train=False, bn_training=True, pfx="encoder.")
        logp = R.decoder_forward(Q, enc, "decoder.decoder_layers.0.", cfg)
        R.ctc_loss_mean_batch(logp, tok, enc_len, tl, cfg.vocab)[0].backward()
        return [enc.detach()] + [Q[k].grad for k in ad] + [enc_len]
    ref, low = run(torch.float64), run(torch.float32)
    out = model.training_step([audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)])
    out["loss"].backward()
    torch.cuda.synchronize()
    assert (model.encoder.packed_last is not None) == packed
    own = dict(model.encoder.named_parameters())
    btd = lambda t: t if t.shape[-1] == 32 else t.transpose(1, 2)
    mask = (torch.arange(btd(ref[0]).shape[1])[None, :] < ref[-1][:, None]).unsqueeze(-1)
    got = [btd(_enc(model, audio, alen).cpu()) * mask] + [own[k[len("encoder."):]].grad.cpu() for k in ad]
    _check(["enc"] + list(ad), got, [btd(ref[0]) * mask] + ref[1:-1], [btd(low[0]) * mask] + low[1:-1])


def test_frozen_base_trains_the_adapters_only():
    model, _, _ = _model()
    model.add_adapter("a", dict(CFG))
    model.freeze()
    model.unfreeze_enabled_adapters()
    assert all(p.requires_grad == (".adapter_layer." in n) for n, p in model.named_parameters())
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    audio, alen, tok, tl = _batch()
    model.setup_optimization(dict(name="adamw", lr=1e-2))
    for _ in range(2):
        model.fit_step([audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)])
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]) != (".adapter_layer." in n), n


def test_bf16_d512_boundary_fused_layers():
    """the configuration the feature is for: bf16 compute, d = 512 (bf16 weight images with their pitches, the fused norm_out / next
    LayerNorm boundary forward and backward).  Zero W_up is the identity to the bit; a frozen-base step moves the adapters alone."""
    model, _, _ = _model(d_model=512, cdt=torch.bfloat16)
    assert model.encoder.fuse_layer_boundary_norms
    model.eval()
    audio, alen, tok, tl = _batch()
    base = _enc(model, audio, alen)
    model.add_adapter("a", dict(CFG, in_features=512, dim=32))
    assert torch.equal(_enc(model, audio, alen), base)
    _randomise(model)
    assert not torch.equal(_enc(model, audio, alen), base)
    model.set_enabled_adapters(enabled=False)
    assert torch.equal(_enc(model, audio, alen), base)
    model.set_enabled_adapters(enabled=True)
    model.freeze()
    model.unfreeze_enabled_adapters()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    model.setup_optimization(dict(name="adamw", lr=1e-2))
    for _ in range(2):
        loss = model.fit_step([audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)])["loss"]
    assert torch.isfinite(loss)
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all() and torch.equal(p, before[n]) != (".adapter_layer." in n), n
