"""-m gpu: the Token-and-Duration Transducer on the MI355X -- csrc/tdt.hip (loss + both gradient parts) against the float64
oracle of tests/tdt_oracle.py, the bf16 pitched gradient operand, the omega mix with the RNN-T loss, the fused joint + loss
against the un-fused joint + TDTLoss + autograd, the greedy TDT search (csrc/rnnt_decode.hip) against its Python restatement,
and the FastConformer-TDT model end to end (training, transcribe, two data-parallel ranks)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tdt_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
dev = "cuda"


def _batch(B, T, U1, W, D, blank, seed):
    g = torch.Generator().manual_seed(seed)
    V1 = W - D
    acts = torch.randn(B, T, U1, W, generator=g) * 2.0
    lens = torch.randint(max(1, T // 2), T + 1, (B,), generator=g); lens[0] = T
    ll = torch.randint(0, U1, (B,), generator=g) if U1 > 1 else torch.zeros(B, dtype=torch.int64)
    ll[-1] = U1 - 1
    if B > 2 and U1 > 1:
        ll[1] = 0   # an empty-label utterance
    labels = torch.randint(0, V1 - 1, (B, max(U1 - 1, 0)), generator=g)
    labels = labels + (labels >= blank).long()
    return acts, labels, lens, ll


@pytest.mark.parametrize("B,T,U1,W,durations", [(3, 9, 6, 7 + 3, [0, 1, 2]), (4, 33, 70, 29 + 5, [0, 1, 2, 3, 4]),
                                                 (2, 250, 90, 1025 + 5, [0, 1, 2, 3, 4]), (3, 12, 5, 8 + 4, [0, 1, 3, 8])])
def test_tdt_loss_matches_the_oracle_on_ragged_batches(B, T, U1, W, durations):
    """loss, label gradient and duration gradient against the float64 oracle: ragged T and U, U1 beyond one wave, an empty-label
    utterance, sigma 0 and 0.05, the none / sum / mean reductions under a non-trivial upstream gradient"""
    from nemo_amd.modules import TDTLoss
    D = len(durations)
    blank = W - D - 1
    acts, labels, lens, ll = _batch(B, T, U1, W, D, blank, B * 1000 + T)
    for red, sigma in (("sum", 0.0), ("mean", 0.05), ("none", 0.05)):
        a = acts.to(dev).requires_grad_(True)
        cost = TDTLoss(blank=blank, durations=durations, reduction=red, sigma=sigma)(a, labels.to(dev), lens.to(dev), ll.to(dev))
        up = torch.linspace(0.5, 1.5, cost.numel(), device=dev)
        (cost * up).sum().backward()
        rc, rg = O.tdt_loss_and_grad(acts, labels, lens, ll, durations, blank, sigma, red)
        upc = up.cpu().double()
        rg = rg * (upc.view(-1, 1, 1, 1) if red == "none" else upc)
        assert torch.allclose(cost.detach().cpu().double(), rc, rtol=2e-5, atol=1e-4), (red, cost, rc)
        tol = 2e-5 if T + U1 < 64 else 1e-3
        ga = a.grad.cpu().double()
        for part in (slice(0, W - D), slice(W - D, W)):   # label and duration columns separately
            err = (ga[..., part] - rg[..., part]).abs().max().item()
            assert err <= tol * max(1.0, rg[..., part].abs().max().item()), (red, part, err)


def test_tdt_bf16_pitched_gradient_is_the_f32_gradient_cast():
    from nemo_amd import ops
    B, T, U1, V1, durations = 3, 17, 9, 1025, [0, 1, 2, 3, 4]
    D = len(durations)
    W = V1 + D
    ld = (W + 7) // 8 * 8
    acts, labels, lens, ll = _batch(B, T, U1, W, D, V1 - 1, 7)
    a = torch.zeros(B * T * U1, ld)
    a[:, :W] = acts.view(-1, W)
    a = a.to(dev)
    lab, el, tl = labels.to(dev), lens.to(dev), ll.to(dev)
    g32 = torch.full((B * T * U1, W), 7.0, device=dev)
    c32 = ops.tdt_loss_pitched(a, ld, B, T, U1, V1, durations, lab, el, tl, V1 - 1, grads=g32, ld_grads=W, sigma=0.02,
                               grad_scale=0.25)
    g16 = torch.full((B * T * U1, ld), 7.0, device=dev, dtype=torch.bfloat16)
    c16 = ops.tdt_loss_pitched(a, ld, B, T, U1, V1, durations, lab, el, tl, V1 - 1, grads=g16, ld_grads=ld, sigma=0.02,
                               grad_scale=0.25)
    torch.cuda.synchronize()
    assert torch.equal(c32, c16)
    assert torch.equal(g16[:, :W], g32.to(torch.bfloat16))
    assert float(g16[:, W:].float().abs().sum()) == 0.0


def test_tdt_omega_mixes_in_the_rnnt_loss_of_the_label_logits():
    from nemo_amd.modules import RNNTLoss, TDTLoss
    B, T, U1, V1, durations = 3, 11, 5, 9, [0, 1, 2]
    D = len(durations)
    acts, labels, lens, ll = _batch(B, T, U1, V1 + D, D, V1 - 1, 3)
    args = (labels.to(dev), lens.to(dev), ll.to(dev))

    def run(mod, x):
        a = x.to(dev).requires_grad_(True)
        c = mod(a, *args)
        c.sum().backward()
        return c.detach().cpu(), a.grad.cpu()

    rn_c, rn_g = run(RNNTLoss(blank=V1 - 1, reduction="sum"), acts[..., :V1].contiguous())
    td_c, td_g = run(TDTLoss(blank=V1 - 1, durations=durations, reduction="sum", sigma=0.05, omega=0.0), acts)
    # (the RNN-T kernels walk rows of pitch V1 + D here and of pitch V1 in RNNTLoss: a different vector / scalar split of the same
    #  arithmetic, so the gradients agree to rounding, the costs exactly)
    same_rnnt = lambda g: torch.allclose(g[..., :V1], rn_g, rtol=1e-6, atol=1e-7) and float(g[..., V1:].abs().sum()) == 0.0
    c1, g1 = run(TDTLoss(blank=V1 - 1, durations=durations, reduction="sum", sigma=0.05, omega=1.0), acts)
    assert torch.equal(c1, rn_c) and same_rnnt(g1)
    c0, g0 = run(TDTLoss(blank=V1 - 1, durations=durations, reduction="sum", sigma=0.05, omega=0.0), acts)
    assert torch.equal(c0, td_c) and torch.equal(g0, td_g) and not torch.allclose(c0, rn_c)
    torch.manual_seed(11)
    mix = TDTLoss(blank=V1 - 1, durations=durations, reduction="sum", sigma=0.05, omega=0.5)
    seen = set()
    for _ in range(12):
        c, g = run(mix, acts)
        if torch.equal(c, rn_c):
            assert same_rnnt(g)
            seen.add("rnnt")
        else:
            assert torch.equal(c, td_c) and torch.equal(g, td_g)
            seen.add("tdt")
    assert seen == {"rnnt", "tdt"}


def _tdt_model(cdt=torch.float32, durations=(0, 1, 2, 3, 4), omega=0.0, d_model=64, **over):
    from nemo_amd.models import EncDecRNNTModel, fastconformer_tdt_config
    enc = dict(d_model=d_model, n_heads=4, n_layers=2, subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0,
               dropout_att=0.0, compute_dtype=cdt)
    enc.update(over)
    cfg = fastconformer_tdt_config("small", vocab_size=30, durations=durations, sigma=0.02, omega=omega, **enc)
    cfg["preprocessor"]["dither"] = 0.0
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    cfg["joint"]["fused_batch_size"] = 2
    m = EncDecRNNTModel(cfg)
    m.decoder.compute_dtype = m.joint.compute_dtype = cdt
    return m


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_fused_tdt_joint_matches_the_unfused_joint_and_autograd(cdt):
    """fuse_loss_wer (sub-batches of 2, ragged lengths: the sub-batch cut engages) against the un-fused joint -> TDTLoss ->
    autograd: the loss, d enc, d dec and the joint's parameter gradients"""
    from oracle import conformer_ref as R
    torch.manual_seed(2)
    m = _tdt_model(cdt).to(dev).train()
    audio, alen, tok, tl = R.synthetic_batch(4, 2.0, vocab=30, seed=12)
    alen = torch.tensor([20000, 16000, 30000, 12000]); tl = torch.tensor([3, 2, 5, 1])
    batch = [audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)]
    res = {}
    for fused in (True, False):
        m.joint.set_fuse_loss_wer(fused, loss=m.loss if fused else None, metric=None)
        for mod in (m.encoder, m.decoder, m.joint):
            mod.flat_parameters().zero_grad()
        loss = m.training_step(batch)["loss"]
        loss.backward()
        m._after_backward()
        torch.cuda.synchronize()
        res[fused] = (loss.item(), {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None})
    tol = 2e-4 if cdt == torch.float32 else 2e-2
    assert abs(res[True][0] - res[False][0]) <= tol * abs(res[False][0]), (res[True][0], res[False][0])
    scale = max(g.norm().item() for g in res[False][1].values())
    assert set(res[True][1]) == set(res[False][1])
    for n, g in res[False][1].items():
        err = (res[True][1][n] - g).norm().item()
        assert err <= tol * max(g.norm().item(), 1e-2 * scale) * (1 if cdt == torch.float32 else 3), (n, err, g.norm().item())
    # the duration rows of the output layer receive gradient
    out = [n for n in res[True][1] if n.startswith("joint.joint_net.") and n.endswith(".weight")][0]
    assert res[True][1][out][-5:].abs().sum().item() > 0


@pytest.mark.parametrize("max_symbols", [10, 2])
def test_greedy_tdt_search_matches_the_restatement(max_symbols):
    """fp32 and bf16 weight images: tokens, frame indices and lengths bit-identical to tests/tdt_oracle.py:tdt_greedy_decode
    (bf16: the restatement on the same bf16-rounded weights and encoder projection); blanks predicted with duration 0 and runs of
    duration-0 labels cut at max_symbols occur"""
    from nemo_amd.modules import GreedyBatchedTDTInfer, RNNTDecoder, RNNTJoint
    torch.manual_seed(5)
    V, H, Denc, J, B, T = 40, 64, 48, 64, 6, 40
    durations = [0, 1, 2, 3, 4]
    dec = RNNTDecoder(prednet={"pred_hidden": H, "pred_rnn_layers": 1, "dropout": 0.0}, vocab_size=V, compute_dtype=torch.float32)
    joint = RNNTJoint(jointnet={"encoder_hidden": Denc, "pred_hidden": H, "joint_hidden": J, "activation": "relu", "dropout": 0.0},
                      num_classes=V, num_extra_outputs=len(durations), compute_dtype=torch.float32)
    with torch.no_grad():
        for p in list(dec.parameters()) + list(joint.parameters()):
            p.mul_(4.0)
        joint.joint_net[-1].bias[V] += 1.0
        joint.joint_net[-1].bias[V + 1] += 3.0   # duration 0 is frequent
    Pd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    Pj = {k: v.detach().clone() for k, v in joint.state_dict().items()}
    enc = torch.randn(B, Denc, T) * 1.5
    enc_len = torch.tensor([40, 31, 0, 40, 7, 1])
    want = O.tdt_greedy_decode(Pd, Pj, enc, enc_len, V, durations, max_symbols)
    dec, joint = dec.to(dev).eval(), joint.to(dev).eval()
    hyps = GreedyBatchedTDTInfer(dec, joint, V, durations, max_symbols_per_step=max_symbols)(
        encoder_output=enc.to(dev), encoded_lengths=enc_len.to(dev))[0]
    assert sum(len(w[0]) for w in want) > 40
    for b, h in enumerate(hyps):
        assert h.y_sequence.tolist() == want[b][0] and h.timestamp == want[b][1], (b, h.y_sequence.tolist(), want[b])
    assert len(hyps[2].y_sequence) == 0
    # some frame holds more than one label (duration 0), and some gap is longer than one frame (a duration > 1)
    steps = [np.diff(w[1]).tolist() for w in want if len(w[1]) > 1]
    assert any(0 in s for s in steps) and any(x > 1 for s in steps for x in s)
    if max_symbols == 2:
        assert any(w[1].count(t) == 2 for w in want for t in set(w[1]))   # the cap ends duration-0 runs
    rb = lambda w: w.to(torch.bfloat16).to(torch.float32)
    Pd16, Pj16 = dict(Pd), dict(Pj)
    for k in ("prediction.dec_rnn.lstm.weight_ih_l0", "prediction.dec_rnn.lstm.weight_hh_l0"):
        Pd16[k] = rb(Pd[k])
    outk = [k for k in Pj if k.startswith("joint_net.") and k.endswith(".weight")][0]
    for k in ("pred.weight", "enc.weight", outk):
        Pj16[k] = rb(Pj[k])
    f16 = rb(torch.nn.functional.linear(rb(enc.transpose(1, 2)), Pj16["enc.weight"], Pj["enc.bias"]))
    want16 = O.tdt_greedy_decode(Pd16, Pj16, enc, enc_len, V, durations, max_symbols, f_all=f16)
    dec.compute_dtype = joint.compute_dtype = torch.bfloat16
    hb = GreedyBatchedTDTInfer(dec, joint, V, durations, max_symbols_per_step=max_symbols)(
        encoder_output=enc.to(dev), encoded_lengths=enc_len.to(dev))[0]
    for b, h in enumerate(hb):
        assert h.y_sequence.tolist() == want16[b][0] and h.timestamp == want16[b][1], b


def test_fastconformer_tdt_model_trains_transcribes_and_bf16_tracks_fp32():
    from oracle import conformer_ref as R
    audio, alen, tok, tl = R.synthetic_batch(4, 2.0, vocab=30, seed=12)
    alen = torch.tensor([32000, 28000, 30000, 20000]); tl = torch.tensor([6, 4, 5, 3])
    batch = [audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)]
    torch.manual_seed(2)
    m32 = _tdt_model(torch.float32, d_model=256, omega=0.1)
    m32._cfg["labels"] = [chr(ord("a") + i) for i in range(26)] + [" ", "'", ".", "-"]
    m32 = m32.to(dev).train()
    m32.setup_optimization(dict(name="adamw", lr=1e-3, betas=[0.9, 0.98], weight_decay=0.0))
    sd = {k: v.clone() for k, v in m32.state_dict().items()}
    m32.loss.omega = 0.0   # the first loss value is compared with bf16 below: a deterministic objective for it
    losses = [m32.fit_step(batch)["loss"].item()]
    m32.loss.omega = 0.1
    losses += [m32.fit_step(batch)["loss"].item() for _ in range(29)]
    assert all(np.isfinite(losses)) and np.mean(losses[-5:]) < 0.7 * losses[0], losses
    texts = m32.transcribe([audio[i, :int(alen[i])].numpy() for i in range(2)], batch_size=2)
    assert len(texts) == 2 and all(isinstance(t, str) for t in texts)
    m16 = _tdt_model(torch.bfloat16, d_model=256)
    m16.load_state_dict(sd)
    m16 = m16.to(dev).train()
    l16 = m16.training_step(batch)["loss"]
    l16.backward()
    torch.cuda.synchronize()
    assert abs(l16.item() - losses[0]) <= 1e-2 * abs(losses[0]), (l16.item(), losses[0])
    for n, p in m16.named_parameters():
        assert torch.isfinite(p.grad).all(), n
    m16.eval()
    v = m16.validation_pass(batch)["val_loss"]
    e = m16.training_step(batch)["loss"]
    torch.cuda.synchronize()
    assert torch.isfinite(v) and abs(v.item() - e.item()) <= 1e-5 * abs(e.item()), (v.item(), e.item())


def _dp_batch():
    from oracle import conformer_ref as R
    audio, alen, tok, tl = R.synthetic_batch(4, 1.0, vocab=30, seed=8)
    return audio, torch.tensor([16000, 12000, 14000, 9000]), tok, torch.tensor([3, 2, 3, 1])


def _dp_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        torch.manual_seed(5)
        model = _tdt_model().to(dev).train()
        model.setup_optimization(dict(name="adamw", lr=1e-3, betas=[0.9, 0.98], weight_decay=0.0))
        audio, alen, tok, tl = _dp_batch()
        sl = slice(2 * rank, 2 * rank + 2)
        batch = [audio[sl].to(dev), alen[sl].to(dev), tok[sl].to(dev), tl[sl].to(dev)]
        syncs = model._grad_syncs()
        model._optimizer.zero_grad()
        loss = model.training_step(batch)["loss"]
        loss.backward()
        model._after_backward()
        scale = 1.0
        for gs in syncs:
            scale = gs.wait()
        torch.cuda.synchronize()
        grads = [fp.grad.detach().cpu() * scale for fp in model.flats()]
        model.fit_step(batch)
        model.fit_step(batch)
        torch.cuda.synchronize()
        torch.save(dict(grads=grads, loss=loss.detach().cpu(), flat=[fp.flat.detach().cpu() for fp in model.flats()]),
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_data_parallel_tdt_two_ranks_equal_one_process_on_the_joint_batch(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt"); r1 = torch.load(tmp_path / "rank1.pt")
    torch.manual_seed(5)
    model = _tdt_model().to(dev).train()
    model.setup_optimization(dict(name="adamw", lr=1e-3, betas=[0.9, 0.98], weight_decay=0.0))
    audio, alen, tok, tl = _dp_batch()
    batch = [audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)]
    model._optimizer.zero_grad()
    loss = model.training_step(batch)["loss"]
    loss.backward()
    model._after_backward()
    torch.cuda.synchronize()
    assert abs(0.5 * (r0["loss"] + r1["loss"]).item() - loss.item()) <= 1e-5 * abs(loss.item())
    for g0, g1, fp in zip(r0["grads"], r1["grads"], model.flats()):
        assert torch.equal(g0, g1)
        ref = fp.grad.detach().cpu()
        assert (g0 - ref).norm() <= 3e-4 * ref.norm(), ((g0 - ref).norm() / ref.norm())
    for a, b in zip(r0["flat"], r1["flat"]):
        assert torch.equal(a, b)
