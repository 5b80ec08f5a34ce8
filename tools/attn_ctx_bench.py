"""Timings behind profiles/attention_ctx.md: the windowed rel-pos flash attention (csrc/attention_ctx.hip) against the GEMM +
soft-max sequence at the cache-aware streaming recipe's geometry, and its forward at long-form lengths against the unlimited
fused forward.  Variants alternate inside one process; medians of device-event times with the 10 % / 90 % quantiles.

    python tools/attn_ctx_bench.py [--out results.json] [--reps 30]
"""
import argparse
import json
import math
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nemo_amd import ops  # noqa: E402
from nemo_amd.modules.conformer_encoder import ConformerEncoder  # noqa: E402

dev, BF16, F32 = "cuda", torch.bfloat16, torch.float32


def timed(variants, reps, warm=5):
    """{name: fn} -> {name: (median ms, q10, q90)}; the variants take turns inside every repetition"""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in variants}
    for _ in range(reps):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1))
    q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]  # noqa: E731
    return {n: (round(q(v, 0.5), 4), round(q(v, 0.1), 4), round(q(v, 0.9), 4)) for n, v in ts.items()}


def recipe_core(T, reps, B=32, H=8, dk=64, win=(70, 13)):
    """attention core of one layer through ConformerEncoder._attn_fwd / _attn_bwd: use_flash_ctx_attention True against False"""
    d = H * dk
    enc = ConformerEncoder(feat_in=80, n_layers=1, d_model=d, n_heads=H, att_context_size=list(win), att_context_style="chunked_limited",
                           dropout=0.0, dropout_att=0.0, compute_dtype=BF16).to(dev)
    enc._pick_ctx()
    enc._saving, enc.dpos_side_stream = True, False
    S = types.SimpleNamespace(cdt=BF16)
    g = torch.Generator().manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    qkv, p, dctx = (0.5 * r(B * T, 3 * d)).to(dev, BF16), (0.5 * r(2 * T - 1, d)).to(dev, BF16), r(B * T, d).to(dev, BF16)
    bu, bv = (0.3 * r(d)).to(dev), (0.3 * r(d)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    dp, dpc, bg = torch.zeros(2 * T - 1, d, device=dev), torch.empty(2 * T - 1, d, dtype=BF16, device=dev), torch.zeros(2 * d, device=dev)

    def fwd(flag):
        enc.use_flash_ctx_attention = flag
        return enc._attn_fwd(S, qkv, p, bu, bv, lens, B, T, d, dk, ops.NO_DROP)

    def both(flag):
        ctx, core = fwd(flag)
        enc._attn_bwd(S, core, qkv, p, bu, bv, ctx, dctx, lens, B, T, d, dk, ops.NO_DROP, dp, dpc, bias_grads=bg if flag else None)

    out = dict(what="recipe attention core", B=B, H=H, dk=dk, T=T, window=list(win), unit="ms (median, q10, q90)")
    out["forward"] = timed({"windowed": lambda: fwd(True), "gemm_softmax": lambda: fwd(False)}, reps)
    out["forward_backward"] = timed({"windowed": lambda: both(True), "gemm_softmax": lambda: both(False)}, reps)
    return out


def long_form(T, reps, H=8, dk=64, w=128):
    """B = 1 forward: local window [w, w] on the windowed kernel, the unlimited fused forward as the dense yardstick"""
    d, B, scale = H * dk, 1, 1.0 / math.sqrt(dk)
    g = torch.Generator().manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    qkv, p = (0.5 * r(T, 3 * d)).to(dev, BF16), (0.5 * r(2 * T - 1, d)).to(dev, BF16)
    bu, bv = (0.3 * r(d)).to(dev), (0.3 * r(d)).to(dev)
    lens = torch.tensor([T], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ctx, lse = torch.empty(T, d, dtype=BF16, device=dev), torch.empty(B, H, T, dtype=F32, device=dev)
    run = lambda win: ops.relpos_flash_fwd(qkv, 3 * d, p, d, bu, bv, lens, ctx, d, lse, B, H, T, dk, (T + 7) // 8 * 8, scale,  # noqa: E731
                                           ctx=win)
    t = timed({"windowed": lambda: run((1, w, w)), "unlimited_flash": lambda: run(None)}, reps)
    return dict(what="long-form forward", B=B, H=H, dk=dk, T=T, window=[w, w], unit="ms (median, q10, q90)", forward=t,
                peak_extra_MiB=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2),
                gemm_path_scores_MiB=round(H * B * T * (T + 2 * T) * 4 / 2 ** 20, 1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    res = []
    for fn, T in [(recipe_core, 250), (recipe_core, 500), (long_form, 2048), (long_form, 8192), (long_form, 32768)]:
        res.append(fn(T, a.reps))
        print(json.dumps(res[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
