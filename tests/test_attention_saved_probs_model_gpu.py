"""-m gpu: one small bf16 Conformer (2 layers, d_model = 512 / 8 heads -> d_k = 64, T' = 63, attention dropout on) differentiated
with `flash_save_probs` on and off.  On: the forward exports its probabilities and dQ / dK/dV read them back
(mi355x_relpos_flash_*_p); off: the recomputing kernels.  Same step counter -> same dropout masks; the two differ by one bf16 rounding of
each attention probability.

Tolerance: the one tests/test_model_gpu.py::test_fused_joint_cuts_sub_batches_to_their_own_lengths applies between two bf16 runs
of one model -- loss within 2e-2 relative, every gradient within 3 * 2e-2 * max(|g|, 1e-2 * the largest gradient norm) in L2."""
import pytest
import torch

from oracle import conformer_ref as R
from test_model_gpu import _model

pytestmark = pytest.mark.gpu

dev = "cuda"


def test_gradients_with_saved_probabilities_match_the_recomputing_backward():
    from nemo_amd import ops
    audio, alen, tok, tl = R.synthetic_batch(3, 2.5, vocab=20, seed=23)
    alen = torch.tensor([40000, 31000, 17000])
    batch = [audio.to(dev), alen.to(dev), tok.to(dev), tl.to(dev)]
    torch.manual_seed(4)
    over = dict(d_model=512, n_heads=8, n_layers=2, dropout=0.0, dropout_pre_encoder=0.0, dropout_att=0.1, compute_dtype=torch.bfloat16)
    m = _model(over, vocab=20)
    m.decoder.compute_dtype = torch.bfloat16
    m = m.to(dev).train()
    enc = m.encoder
    assert enc.flash_save_probs in (True, False) and enc._geometry(torch.bfloat16)[1] == 64
    calls = {"fwd_p": 0, "dq_p": 0, "dkv_p": 0, "dq": 0, "dkv": 0}
    real = {n: getattr(ops, n) for n in ("relpos_flash_fwd_p", "relpos_flash_bwd_dq_p", "relpos_flash_bwd_dkv_p", "relpos_flash_bwd_dq",
                                         "relpos_flash_bwd_dkv")}

    def counted(key, fn):
        def f(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return f

    res = {}
    try:
        for key, n in zip(calls, real):
            setattr(ops, n, counted(key, real[n]))
        for on in (False, True):
            enc.flash_save_probs = on
            for mod in m.trainable_modules():
                mod.flat_parameters().zero_grad()
            enc._step_seed = 100      # the step's dropout masks are a function of this counter: the same in both runs
            torch.manual_seed(11)
            before = dict(calls)
            loss = m.training_step(batch)["loss"]
            loss.backward()
            torch.cuda.synchronize()
            took = {k: calls[k] - before[k] for k in calls}
            assert took == (dict(fwd_p=2, dq_p=2, dkv_p=2, dq=0, dkv=0) if on else dict(fwd_p=0, dq_p=0, dkv_p=0, dq=2, dkv=2)), took
            res[on] = (loss.item(), {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None})
    finally:
        for n, fn in real.items():
            setattr(ops, n, fn)
    tol = 2e-2
    print(f"loss: recomputed {res[False][0]!r}, saved probabilities {res[True][0]!r}")
    assert abs(res[True][0] - res[False][0]) <= tol * abs(res[False][0]), (res[True][0], res[False][0])
    scale = max(g.norm().item() for g in res[False][1].values())
    worst = ("", 0.0)
    for n, g in res[False][1].items():
        err = (res[True][1][n] - g).norm().item()
        bound = tol * max(g.norm().item(), 1e-2 * scale) * 3
        if err / bound > worst[1]:
            worst = (n, err / bound)
        assert err <= bound, (n, err, g.norm().item())
    print(f"worst gradient: {worst[0]} at {worst[1]:.3f} x its bound")
    assert any((res[True][1][n] != g).any() for n, g in res[False][1].items()), "the two paths gave identical bits: one of them did not run"
