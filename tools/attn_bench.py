"""per-kernel timing of the fused rel-pos attention kernels at the Conformer-CTC-Large shape (B=32, H=8, T=501, dk=64)"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nemo_amd import ops
dev = "cuda"
B, H, T, dk = 32, 8, 501, 64
d = H * dk; Tp = (T + 7) // 8 * 8; scale = 1 / math.sqrt(dk)
g = torch.Generator(device=dev).manual_seed(0)
bf = torch.bfloat16
qkv = (torch.randn(B * T, 3 * d, device=dev, generator=g) * 0.5).to(bf)
pos = (torch.randn(2 * T - 1, d, device=dev, generator=g) * 0.5).to(bf)
u = torch.randn(d, device=dev, generator=g) * 0.1; v = torch.randn(d, device=dev, generator=g) * 0.1
lens = torch.full((B,), 500, device=dev, dtype=torch.int64)
dO = torch.randn(B * T, d, device=dev, generator=g).to(bf)
ctx = torch.empty(B * T, d, device=dev, dtype=bf); lse = torch.zeros(B, H, T, device=dev)
qu = torch.empty(B * T, d, device=dev, dtype=bf); qv = torch.empty_like(qu)
dlt = torch.zeros(B, H, T, device=dev)
dqu = torch.empty_like(qu); dqv = torch.empty_like(qu)
dqkv = torch.empty(B * T, 3 * d, device=dev, dtype=bf)
dp = torch.zeros(2 * T - 1, d, device=dev)
drop = ops.Dropout(0.1, 1, 2)
REPS = int(os.environ.get("ATTN_BENCH_REPS", "5"))   # repetitions of 10 launches each: min / median are printed
def t(name, fn, flops):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10): fn()
        e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / 10 * 1e3)
    us.sort()
    print(f"{name:12s} min {us[0]:8.1f} us  median {us[len(us) // 2]:8.1f} us  max {us[-1]:8.1f} us   {flops / us[0] / 1e6:7.1f} TFLOP/s (useful, at min)", flush=True)
pair = 2.0 * B * H * T * T * dk  # one T x T x dk product
t("fwd", lambda: ops.relpos_flash_fwd(qkv, 3 * d, pos, d, u, v, lens, ctx, d, lse, B, H, T, dk, Tp, scale, drop), 3 * pair)
ctx_lo = torch.empty_like(ctx)
t("prep", lambda: ops.attn_bwd_prep(dO, ctx, dlt, qkv, 3 * d, u, v, qu, qv, B, H, T, d, O_lo=ctx_lo), 0.0)
ops.qbias(qkv, 3 * d, u, v, qu, qv, B * T, d); ops.attn_delta(dO, ctx, dlt, B, H, T, d)
dS = ops.relpos_ds_buffer(B, H, T, dev, fill=0.0)
t("bwd_dq", lambda: ops.relpos_flash_bwd_dq(qu, qv, qkv, 3 * d, pos, d, lens, dO, lse, dlt, dqu, dqv, B, H, T, dk, scale, drop, ds_out=dS), 5 * pair)
t("bwd_dkv", lambda: ops.relpos_flash_bwd_dkv(qu, qv, qkv, 3 * d, pos, d, lens, dO, lse, dlt, dqkv, 3 * d, B, H, T, dk, Tp, scale, drop), 5 * pair)
t("bwd_dpos", lambda: ops.relpos_flash_bwd_dpos(qv, dS, lens, dp, B, H, T, dk), 1 * pair)
# the saved-probabilities variants (MI355X_ATTN_SAVE_P=1): the forward exports p~ / mref, dQ and dK/dV read them back
probs = torch.empty(ops.lib.mi355x_relpos_probs_elems(B, H, T), device=dev, dtype=bf)
mref = torch.empty(ops.lib.mi355x_relpos_mref_elems(B, H, T), device=dev)
t("fwd_p", lambda: ops.relpos_flash_fwd_p(qkv, 3 * d, pos, d, u, v, lens, ctx, d, lse, probs, mref, B, H, T, dk, Tp, scale, drop), 3 * pair)
t("bwd_dq_p", lambda: ops.relpos_flash_bwd_dq_p(probs, mref, qkv, 3 * d, pos, d, lens, dO, lse, dlt, dqu, dqv, B, H, T, dk, scale, drop, ds_out=dS), 3 * pair)
t("bwd_dkv_p", lambda: ops.relpos_flash_bwd_dkv_p(probs, mref, qu, qkv, 3 * d, lens, dO, lse, dlt, dqkv, 3 * d, B, H, T, dk, scale, drop), 3 * pair)
