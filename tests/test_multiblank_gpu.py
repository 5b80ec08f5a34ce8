"""-m gpu: csrc/multiblank.hip and the multi-blank mode of the greedy search against the float64 restatement of tests/multiblank_oracle.py,
and a tiny model end to end.  The tolerance is the project's rule: max(8 x |float32 restatement - float64|, 16 ulp)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiblank_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
dev = "cuda"
DUR = [2, 4, 8]
ulp16 = lambda ref: 16 * np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64)

# (T, U, V, act_lens, label_lens, misalign): T_b = 1, T_b = 8 with U_b = 0 (one d = 8 arc is a whole path), U_b = U; N = 1028 on rows 4
# bytes off a 16-byte boundary (vector walk with a head); U1 = 71 (the label neighbour crosses a wave border)
CASES = {"edges": (9, 4, 5, [9, 1, 8, 6], [4, 2, 0, 3], 0), "n1028": (5, 3, 1024, [5, 3], [3, 1], 1),
         "two_waves": (10, 70, 5, [10, 7], [70, 33], 0)}
_refs = {}


def _case(name, sigma):
    """inputs and the float64 / float32 restatements, computed once"""
    if (name, sigma) not in _refs:
        T, U, V, el, tl, _ = CASES[name]
        g = torch.Generator().manual_seed(len(name) * 100 + T)
        acts = torch.randn(len(el), T, U + 1, V + 1 + len(DUR), generator=g) * 2.0
        labels = torch.randint(0, V, (len(el), U), generator=g)
        el, tl = torch.tensor(el), torch.tensor(tl)
        _refs[name, sigma] = (acts, labels, el, tl, O.loss_and_grad(acts, labels, el, tl, DUR, sigma),
                              O.loss_and_grad(acts, labels, el, tl, DUR, sigma, torch.float32))
    return _refs[name, sigma]


def _offset(t, k):   # a copy of t on the device that starts k floats behind a 16-byte boundary
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
    buf[k:k + t.numel()] = t.reshape(-1).to(dev)
    return buf[k:k + t.numel()].view(t.shape)


@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradient_against_float64(name, sigma):
    from nemo_amd import ops
    acts, labels, el, tl, (c64, g64), (c32, g32) = _case(name, sigma)
    a = _offset(acts, CASES[name][5])
    grads = _offset(torch.full_like(acts, float("nan")), CASES[name][5])
    costs = ops.multiblank_loss(a, labels.to(dev), el.to(dev), tl.to(dev), acts.shape[-1] - 1, DUR, grads=grads, sigma=sigma)
    _within_the_rule(name, costs, grads, c64, g64, c32, g32)
    assert all(not grads[b, int(el[b]):].any() and not grads[b, :, int(tl[b]) + 1:].any() for b in range(len(el)))   # padded: zeros


def _within_the_rule(what, costs, grads, c64, g64, c32, g32, scale=1.0):   # (`scale`: the grad_scale of the call)
    cerr, gerr = (costs.cpu().double() - c64).abs(), (grads.cpu().double() - scale * g64).abs()
    ctol = np.maximum(8 * (c32.double() - c64).abs().numpy(), ulp16(c64))
    gtol = np.maximum(8 * scale * float((g32.double() - g64).abs().max()), ulp16(scale * g64))
    print(what, "cost err / tol", float((cerr.numpy() / ctol).max()), "grad err / tol", float((gerr.numpy() / gtol).max()))
    assert (cerr.numpy() <= ctol).all(), (cerr, ctol)
    assert (gerr.numpy() <= gtol).all(), float((gerr.numpy() / gtol).max())


def test_bf16_pitched_gradient_is_the_f32_gradient_cast():
    from nemo_amd import ops
    acts, labels, el, tl, (c64, g64), (c32_ref, g32_ref) = _case("edges", 0.05)
    B, T, U1, N = acts.shape
    ld = 16
    a = torch.zeros(B, T, U1, ld, device=dev)
    a[..., :N] = acts.to(dev)
    lab, el, tl = labels.to(dev), el.to(dev), tl.to(dev)
    run = lambda g: ops.multiblank_loss_pitched(a, ld, B, T, U1, N, DUR, lab, el, tl, N - 1, grads=g, ld_grads=ld, sigma=0.05,
                                                grad_scale=0.5)   # (the same rows and pitch: the same walk, so the same bits)
    g32 = torch.full((B, T, U1, ld), float("nan"), device=dev)
    g16 = torch.full((B, T, U1, ld), float("nan"), device=dev, dtype=torch.bfloat16)
    c32, c16 = run(g32), run(g16)
    _within_the_rule("pitched", c32, g32[..., :N], c64, g64, c32_ref, g32_ref, scale=0.5)   # the f32 rows of pitch 16: the rule
    assert torch.equal(c16, c32) and torch.equal(g16[..., :N], g32[..., :N].to(torch.bfloat16)) and not (g16[..., N:].any() or g32[..., N:].any())


H, J, V, T, LENS, MAX_SYM = 40, 24, 9, 12, (12, 7, 0), 2
SEED = {"fp32": 1, "bf16": 1}   # the first of 0, 1, 2, ... whose float64 runs meet the case condition asserted below


def _greedy_weights(seed, bf16):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k
    m = dict(emb=r(V + 1, H), w_ih=r(4 * H, H, k=0.3), w_hh=r(4 * H, H, k=0.3), b_ih=r(4 * H, k=0.1), b_hh=r(4 * H, k=0.1),
             w_pred=r(J, H, k=0.3), b_pred=r(J, k=0.1), w_out=r(V + 1 + len(DUR), J, k=0.5), b_out=r(V + 1 + len(DUR), k=0.1))
    m["emb"][V] = 0.0
    m["b_out"][V:V + len(DUR)] += 0.3   # the big-blank rows: jumps happen
    f = r(len(LENS), T, J)
    if bf16:   # the images: bf16-representable weights and encoder projection
        for k in ("w_ih", "w_hh", "w_pred", "w_out"):
            m[k] = m[k].to(torch.bfloat16).float()
        f = f.to(torch.bfloat16).float()
    return m, f


@pytest.mark.parametrize("image", ["fp32", "bf16"])
def test_greedy_search_against_the_float64_rule(image):
    from nemo_amd import ops
    bf16 = image == "bf16"
    m, f = _greedy_weights(SEED[image], bf16)
    mn = {k: v.numpy() for k, v in m.items()}
    r64 = [O.greedy(mn, f[b].numpy(), n, DUR, MAX_SYM) for b, n in enumerate(LENS)]
    r32 = [O.greedy(mn, f[b].numpy(), n, DUR, MAX_SYM, np.float32) for b, n in enumerate(LENS)]
    # the case condition, from the references alone: margins, big blanks and labels, a jump past an end and one across a cut
    jumps = [(b, t, d) for b, r in enumerate(r64) for t, d in r["jumps"]]
    assert min(r["margin"] for r in r64) >= 1e-3 and jumps and all(len(r["tokens"]) >= 2 for r in r64[:2])
    assert any(t + d > LENS[b] for b, t, d in jumps)
    assert any(t < cut < t + d for b, t, d in jumps for cut in (5, 3, 6, 9) if cut < LENS[b])
    wd = torch.bfloat16 if bf16 else torch.float32
    d = {k: v.to(dev).to(wd if k.startswith("w_") else torch.float32).contiguous() for k, v in m.items()}
    args = (d["emb"], d["w_ih"], H, d["w_hh"], H, d["b_ih"], d["b_hh"], d["w_pred"], H, d["b_pred"], d["w_out"], J, d["b_out"], V, DUR,
            MAX_SYM)
    fd, lens = f.to(dev).to(wd).contiguous(), torch.tensor(LENS, device=dev)
    tokens, times, out_len, score = (t.cpu() for t in ops.multiblank_greedy_decode(fd, lens, *args))
    for b, (a, e) in enumerate(zip(r64, r32)):
        n = int(out_len[b])
        assert tokens[b, :n].tolist() == a["tokens"] and times[b, :n].tolist() == a["frames"] and (tokens[b, n:] == -1).all()
        tol = max(8 * abs(e["score"] - a["score"]), 16 * float(np.spacing(np.float32(abs(a["score"])))))
        print(image, b, "score err / tol", abs(float(score[b]) - a["score"]) / tol if tol else 0.0)
        assert abs(float(score[b]) - a["score"]) <= tol
    for cuts in [(12,), (5, 7), (3, 3, 3, 3)]:   # the resumable form: the bits of one launch
        state, t0, tok, frm = None, 0, [[] for _ in LENS], [[] for _ in LENS]
        for n in cuts:
            cl = (lens - t0).clamp(0, n)
            tk, tm, ol, state = ops.multiblank_greedy_decode_stream(fd[:, t0:t0 + n].contiguous(), cl, *args, state=state)
            for b in range(len(LENS)):
                tok[b] += tk[b, :int(ol[b])].tolist(); frm[b] += tm[b, :int(ol[b])].tolist()
            t0 += n
        assert tok == [r["tokens"] for r in r64] and frm == [r["frames"] for r in r64], cuts
        assert torch.equal(state.score.cpu(), score) and not state.zero_run.any(), cuts


def test_a_tiny_model_trains_and_transcribes():
    from nemo_amd.models import EncDecRNNTModel, fastconformer_multiblank_config
    from nemo_amd.modules import GreedyBatchedMultiblankRNNTInfer
    from oracle import conformer_ref as R
    cfg = fastconformer_multiblank_config("small", vocab_size=30, big_blank_durations=DUR, d_model=64, n_heads=4, n_layers=1,
                                          subsampling_conv_channels=32, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.0)
    cfg["preprocessor"]["dither"] = 0.0
    cfg["labels"] = [chr(ord("a") + i) for i in range(26)] + [" ", "'", ".", "-"]
    cfg["decoder"]["prednet"].update(pred_hidden=64, dropout=0.0)
    cfg["joint"]["jointnet"].update(joint_hidden=64, dropout=0.0)
    cfg["joint"]["fused_batch_size"] = 2
    torch.manual_seed(2)
    m = EncDecRNNTModel(cfg).to(dev).train()
    audio, alen, tok, tl = R.synthetic_batch(4, 2.0, vocab=30, seed=12)
    alen, tl = torch.tensor([20000, 16000, 30000, 12000]), torch.tensor([3, 2, 5, 1])
    loss = m.training_step([audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)])["loss"]
    loss.backward()
    m._after_backward()
    out = m.joint.joint_net[-1]
    assert out.weight.shape[0] == 30 + 1 + len(DUR) and torch.isfinite(loss)
    assert out.weight.grad[30:30 + len(DUR)].abs().sum() > 0 and out.bias.grad[30:30 + len(DUR)].abs().sum() > 0
    assert type(m.decoding.decoding) is GreedyBatchedMultiblankRNNTInfer
    texts = m.transcribe([audio[i, :int(alen[i])].numpy() for i in range(2)], batch_size=2)
    assert len(texts) == 2 and all(isinstance(t, str) for t in texts)
